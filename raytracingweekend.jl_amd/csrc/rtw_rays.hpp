// rtw_rays.hpp -- the ray-query kernel: the closest hit of caller-supplied rays against the whole sphere list (include/rtw_hip.h rtw_cast_rays_*).
// gfx950 only; wave = 64 lanes.
//
// The rays come from HBM, 8 elements each (ox oy oz dx dy dz tmax tag), and go through the scans of the trace and feature kernels as they
// stand: hit_world_mfma over the plain scan's own sphere order (scene.orig: ties by the caller's index, and the way back to it), or hit_world
// over the caller's order.  Nothing of a path is run: the result is the index and, where asked for, make_hitrec's record.
//
// Work decomposition: ONE plain kernel with a persistent grid, no queue.
//   workgroup = RTW_RAYS_WAVES waves; the scene is staged ONCE per workgroup, and behind that barrier there is no other;
//   wave      = walks batches of 64 consecutive rays with a grid stride, batch (blockIdx.x * RTW_RAYS_WAVES + wave) + k * RTW_RAYS_WAVES *
//               gridDim.x: the trip count is wave-uniform, every lane calls the (wave-cooperative) matrix-pipe scan in every trip, lanes
//               behind the last ray with has_ray = false;
//   lane      = ray 64 batch + lane: two (Float32) / four (Float64) 16-byte loads -- the wave reads 2 / 4 KB contiguous --, one dword and
//               two / four 16-byte stores.
// tmax.  Both scans run UNBOUNDED (tmax = +inf: the matrix-pipe scan has no other form) and the ray's own tmax is applied to the winner: a
// hit with tmax < t becomes a miss.  That is the reference's bounded scan (closest starts at tmax; a root is rejected when root < tmin ||
// closest < root): a sphere's near root is never above its far root, so a sphere contributes its first root >= tmin or nothing in both
// scans, the bounded one keeps the least of those that are <= tmax -- the later sphere among equals -- and that one is the unbounded
// scan's winner iff the winner is <= tmax.  (tests/test_rays_ref.py asserts the equivalence on the oracle, ray by ray.)
// Directions.  The filter value of hit_world_mfma is an algebraic identity in d (no unit-length assumption) and every term of its error
// budget is bounded through |d|^2 <= 1.001 from ABOVE only: the splits' relative errors scale with the features, the f16 floors are
// absolute, |p| <= |o| holds for every |d|^2 <= 2.  A direction shorter than 1 -- the zero vector included -- therefore keeps the filter a
// superset and needs no other route; a longer one (|d|^2 > 1.0009) or an origin beyond mf_o_max makes the lane "not ok" inside the scan:
// every sphere becomes a candidate of the exact test, slow and correct.  The Float64 VALU filter (hit_world) is bounded the same way.
#pragma once
#include "rtw_device.hpp"
#include "rtw_kernels.hpp"      // DevCounters, lane_id

namespace rtw {

#define RTW_RAYS_WAVES 4        // waves per workgroup
#define RTW_RAY_ELEMS 8         // elements of a ray and of a record

struct RayParams {
    unsigned n;                 // rays (< 2^31)
    unsigned n_batches;         // ceil(n / 64)
};

// LDS of a workgroup: the feature kernel's without the camera -- [candidate lists: per-lane lists of the all-VALU scan / per-wave pair lists
// of the matrix-pipe scan][result cells of the matrix-pipe scan: keys, kidx][scene copy + (matrix pipe) its index array: LDS_SCENE only];
// every offset a multiple of 16
__host__ __device__ constexpr size_t rays_list_bytes() { return (size_t)RTW_LIST_CAP * 64 * RTW_RAYS_WAVES * sizeof(unsigned short); }
__host__ __device__ constexpr size_t rays_cell_bytes() { return (size_t)RTW_RAYS_WAVES * 64 * (sizeof(unsigned long long) + sizeof(unsigned)); }
__host__ __device__ constexpr size_t rays_fixed_lds_bytes() { return rays_list_bytes() + rays_cell_bytes(); }

// waves per SIMD the kernel is compiled for: the scan's own registers and a ray (profiles/rays_kernel_resources.txt)
template <typename T> struct RayWaves { static constexpr int value = 4; };
template <> struct RayWaves<double> { static constexpr int value = 3; };

// a ray's elements 0-5 and its tmax; the tag is loaded with its 16 bytes and never looked at
template <typename T> __device__ __forceinline__ void ray_load(const T *p, V3<T> &o, V3<T> &d, T &tmax);
template <> __device__ __forceinline__ void ray_load<float>(const float *p, V3<float> &o, V3<float> &d, float &tmax) {
    const float4 *q = reinterpret_cast<const float4 *>(p);
    const float4 a = q[0], b = q[1];
    o = {a.x, a.y, a.z}; d = {a.w, b.x, b.y}; tmax = b.z;
}
template <> __device__ __forceinline__ void ray_load<double>(const double *p, V3<double> &o, V3<double> &d, double &tmax) {
    const double2 *q = reinterpret_cast<const double2 *>(p);
    const double2 a = q[0], b = q[1], c = q[2], e = q[3];
    o = {a.x, a.y, b.x}; d = {b.y, c.x, c.y}; tmax = e.x;
}
template <typename T> __device__ __forceinline__ void rec_store(T *o, const T (&r)[RTW_RAY_ELEMS]);
template <> __device__ __forceinline__ void rec_store<float>(float *o, const float (&r)[RTW_RAY_ELEMS]) {
    float4 *q = reinterpret_cast<float4 *>(o);
    q[0] = float4{r[0], r[1], r[2], r[3]};
    q[1] = float4{r[4], r[5], r[6], r[7]};
}
template <> __device__ __forceinline__ void rec_store<double>(double *o, const double (&r)[RTW_RAY_ELEMS]) {
    double2 *q = reinterpret_cast<double2 *>(o);
    q[0] = double2{r[0], r[1]}; q[1] = double2{r[2], r[3]};
    q[2] = double2{r[4], r[5]}; q[3] = double2{r[6], r[7]};
}

// MFMA: hit_world_mfma over the plain scan's own sphere order; otherwise hit_world over the caller's order.  Either way `scene`'s geom /
// mat0 are the arrays the scan's index refers to.  The numerics mode is the one in `scene` (a kernel argument).  rec_out null: no records.
template <typename T, bool MFMA, bool LDS_SCENE>
__global__ __launch_bounds__(64 * RTW_RAYS_WAVES, (RayWaves<T>::value)) void cast_rays_kernel(RayParams P, T tmin, DevScene<T> scene, const T *__restrict__ rays,
                                                                                          int *__restrict__ idx_out, T *__restrict__ rec_out, DevCounters *ctr) {
    using V4 = typename Vec4<T>::type;
    const unsigned lane = lane_id(), wv = threadIdx.x >> 6;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    [[maybe_unused]] unsigned short *my_list = reinterpret_cast<unsigned short *>(smem) + threadIdx.x;
    unsigned char *cells = smem + rays_list_bytes();
    V4 *lds_geom = reinterpret_cast<V4 *>(smem + rays_fixed_lds_bytes());
    [[maybe_unused]] unsigned short *lds_orig = reinterpret_cast<unsigned short *>(lds_geom + scene_geom_alloc(scene.n, scene.n_pad));
    [[maybe_unused]] WaveScratch ws = {nullptr, nullptr, nullptr};
    if constexpr (MFMA) {
        static_assert(rays_list_bytes() == RTW_RAYS_WAVES * RTW_PAIR_CAP * sizeof(unsigned), "the pair lists use the per-lane list area");
        ws.pairs = reinterpret_cast<unsigned *>(smem) + wv * RTW_PAIR_CAP;
        ws.keys = reinterpret_cast<unsigned long long *>(cells) + wv * 64;
        ws.kidx = reinterpret_cast<unsigned *>(cells + RTW_RAYS_WAVES * 64 * sizeof(unsigned long long)) + wv * 64;
    }
    if constexpr (LDS_SCENE) {
        stage_scene<T>(scene, lds_geom);
        if constexpr (MFMA) { for (int i = threadIdx.x; i < scene_geom_alloc(scene.n, scene.n_pad); i += blockDim.x) lds_orig[i] = scene.orig[i]; }
        __syncthreads();
    }
    // (no workgroup barrier from here on: a wave without a batch leaves)
    const unsigned first = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * RTW_RAYS_WAVES + wv)), stride = RTW_RAYS_WAVES * gridDim.x;
    unsigned long long scanned = 0;                                   // rays of this wave's batches (wave-uniform)
#pragma unroll 1
    for (unsigned long long b = first; b < P.n_batches; b += stride) {
        const unsigned i = (unsigned)b * 64u + lane;                  // (n < 2^31: no wrap)
        const bool has = i < P.n;
        V3<T> ro = {0, 0, 0}, rd = {0, 0, 1};
        T tmax = 0;
        if (has) ray_load<T>(rays + (size_t)i * RTW_RAY_ELEMS, ro, rd, tmax);
        T t_hit = 0;
        int idx = -1;
        if constexpr (MFMA) {
            if (LDS_SCENE) idx = hit_world_mfma<T, const V4 *, const unsigned short *, NoClock, NoSink, false>(scene, (const V4 *)lds_geom, ro, rd, has, tmin, t_hit, ws, lane, NoClock(), nullptr, (const unsigned short *)lds_orig);
            else idx = hit_world_mfma<T, const V4 *, const unsigned short *, NoClock, NoSink, false>(scene, scene.geom, ro, rd, has, tmin, t_hit, ws, lane, NoClock(), nullptr, scene.orig);
        } else if (has) {
            if (LDS_SCENE) idx = hit_world<T, 64 * RTW_RAYS_WAVES>(scene, (const V4 *)lds_geom, ro, rd, tmin, (T)__builtin_huge_val(), t_hit, my_list);
            else idx = hit_world<T, 64 * RTW_RAYS_WAVES>(scene, scene.geom, ro, rd, tmin, (T)__builtin_huge_val(), t_hit, my_list);
        }
        if (has) {
            T r[RTW_RAY_ELEMS] = {0, 0, 0, 0, 0, 0, 0, 0};
            int who = -1;
            if (idx >= 0 && !(tmax < t_hit)) {            // the ray's own tmax, applied to the unbounded scan's winner
                const V4 g = scene.geom[idx];             // the scan's own order: what its index refers to
                const V4 m0 = scene.mat0[idx];
                HitRec<T> rec;
                make_hitrec<T>({g.x, g.y, g.z}, m0.x, ro, rd, t_hit, rec);
                r[0] = rec.t; r[1] = rec.p.x; r[2] = rec.p.y; r[3] = rec.p.z;
                r[4] = rec.n.x; r[5] = rec.n.y; r[6] = rec.n.z; r[7] = rec.front ? T(1) : T(0);
                if constexpr (MFMA) who = (int)scene.orig[idx];       // the caller's index
                else who = idx;
            }
            idx_out[i] = who;
            if (rec_out) rec_store<T>(rec_out + (size_t)i * RTW_RAY_ELEMS, r);
        }
        scanned += (unsigned long long)__popcll(__ballot(has));
    }
    // what rtw_stats() reports: one scan per ray (two adds per wave, at the end of its walk)
    if (lane == 0 && scanned != 0ull) {
        atomicAdd(&ctr->segments, scanned);
        atomicAdd(&ctr->samples, scanned);
    }
}

}  // namespace rtw
