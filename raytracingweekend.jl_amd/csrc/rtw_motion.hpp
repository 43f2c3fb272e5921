// rtw_motion.hpp -- the kernel of the first-hit motion pass (include/rtw_hip.h rtw_first_hit_motion_*: the definition is there): per pixel, which
// sphere its centre ray sees and how far that sphere moved since the previous frame.  gfx950 only; wave = 64 lanes.
//   motion_pass    one pixel per lane, 256-lane workgroups, lane = flat pixel P = j*H + i as in tp_step.  The ray is the temporal step's own
//                  (su, tv, D, nD of rtw_temporal.hpp: origin cam.origin, direction nD, no lens), NOT a sample of the trace kernel.  Every lane
//                  walks ALL spheres in the caller's order with a wave-uniform trip count and applies the scan's own exact test -- sphere_disc_n
//                  in the render's numerics mode and sphere_root (rtw_path.hpp), tmin = 1e-4, tmax = +inf -- to each; a sphere replaces the
//                  running hit only with a strictly smaller root, so the smallest t wins and ties stay with the lower caller's index.  There
//                  is no filter pass and no candidate list: a 485-sphere scene is ~20 VALU instructions per sphere and lane, nothing per hit
//                  but two moves, and the pass runs once per frame (DESIGN.md 7.23 has the time next to the feature pass's).
//   LDS_SCENE      true: the workgroup stages the n geometry rows (cx, cy, cz, r*r) into LDS once and every lane reads row k at the same
//                  address (a broadcast read); false (more than RTW_LDS_SCENE_MAX_BYTES of rows: 1528 Float32 / 760 Float64 spheres): row k
//                  comes through the constant address space -- the address is wave-uniform, so the loads are scalar (SMEM) loads.  The radius
//                  itself (mat0[k].x), which only NUM_REFERENCE_FMA2 reads, always comes through scalar loads.
//   store          one slot (m.x, m.y, m.z, id) per lane: 16 bytes (Float32) / 32 bytes (Float64); a hit of sphere k gathers row k of the
//                  motion table (n rows of 4 elements, the caller's order; null: m = 0), a miss stores (0, 0, 0, -1).
// One barrier (behind the staging; lanes past the last pixel leave behind it), no atomics, no cross-lane operation but t_sqrt's wave vote.
#pragma once
#include "rtw_device.hpp"
#include "rtw_denoise.hpp"      // DnVec, dn_sqrt

namespace rtw {

// the camera fields the ray reads and the frame, by value
template <typename T> struct MoParams {
    T o[3], llc[3], hor[3], ver[3];
    int W, H;
};

// row k of a 4-element-per-row array through scalar loads (k is wave-uniform)
template <typename T>
__device__ __forceinline__ typename Vec4<T>::type mo_uniform_row(const typename Vec4<T>::type *rows, int k) {
    typedef const T __attribute__((address_space(4))) *cptr;
    cptr g = (cptr)(uintptr_t)rows;
    typename Vec4<T>::type r;
    r.x = g[4 * k + 0]; r.y = g[4 * k + 1]; r.z = g[4 * k + 2]; r.w = g[4 * k + 3];
    return r;
}

template <typename T, bool LDS_SCENE>
__global__ __launch_bounds__(256) void motion_pass(MoParams<T> U, DevScene<T> scene, const typename DnVec<T>::type *__restrict__ table,
                                                   typename DnVec<T>::type *__restrict__ motion) {
    using V = typename DnVec<T>::type;
    using V4 = typename Vec4<T>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    [[maybe_unused]] V4 *lds_geom = reinterpret_cast<V4 *>(smem);
    const int n = scene.n;
    if constexpr (LDS_SCENE) {
        for (int k = threadIdx.x; k < n; k += 256) lds_geom[k] = scene.geom[k];
        __syncthreads();
    }
    const long long H = U.H, W = U.W, n_pix = W * H;
    const long long P = (long long)blockIdx.x * 256 + threadIdx.x;
    if (P >= n_pix) return;
    long long j, i;
    if (n_pix < (1ll << 31)) {
        const unsigned jj = (unsigned)P / (unsigned)H;
        j = jj; i = (unsigned)P - jj * (unsigned)H;
    } else {
        j = P / H; i = P - j * H;
    }
    // ---- the pixel's own ray: the temporal step's (rtw_temporal.hpp), operation for operation
    const T su = (T((int)j) + T(1.5)) / T((int)W);
    const T tv = (T((int)(H - i)) - T(0.5)) / T((int)H);
    const T D0 = ((U.llc[0] + su * U.hor[0]) + tv * U.ver[0]) - U.o[0];
    const T D1 = ((U.llc[1] + su * U.hor[1]) + tv * U.ver[1]) - U.o[1];
    const T D2 = ((U.llc[2] + su * U.hor[2]) + tv * U.ver[2]) - U.o[2];
    const T sl = dn_sqrt((D0 * D0 + D1 * D1) + D2 * D2);
    const V3<T> o = {U.o[0], U.o[1], U.o[2]}, d = {D0 / sl, D1 / sl, D2 / sl};
    // ---- the first hit: every sphere, the caller's order, a strictly smaller root replaces
    const T tmin = (T)1e-4;
    T closest = (T)__builtin_huge_val();
    int idx = -1;
    auto scan = [&](auto tag) {
        constexpr int NUM = decltype(tag)::value;
        for (int k = 0; k < n; ++k) {
            V4 s;
            if constexpr (LDS_SCENE) s = lds_geom[k];
            else s = mo_uniform_row<T>(scene.geom, k);
            T r = T(0);
            if constexpr (NUM == NUM_REFERENCE_FMA2) r = mo_uniform_row<T>(scene.mat0, k).x;      // (the radius itself)
            T hb, disc, root;
            sphere_disc_n<T, NUM>(s.x, s.y, s.z, s.w, r, o, d, hb, disc);
            if (sphere_root<T>(hb, disc, tmin, closest, root) && root < closest) { closest = root; idx = k; }
        }
    };
    // (the numerics mode is a kernel argument: one scalar branch, the loop once per mode)
    if (scene.numerics == NUM_REFERENCE) scan(NumTag<NUM_REFERENCE>{});
    else if (scene.numerics == NUM_CONTRACT) scan(NumTag<NUM_CONTRACT>{});
    else scan(NumTag<NUM_REFERENCE_FMA2>{});
    // ---- the slot
    V m;
    m.x = T(0); m.y = T(0); m.z = T(0); m.w = T(-1);
    if (idx >= 0) {
        if (table) m = table[idx];
        m.w = T(idx);
    }
    motion[P] = m;
}

}  // namespace rtw
