// rtw_units.hpp -- unit-level device entry points for the T0 parity tier: one lane evaluates
// one reference function on one input, using exactly the device functions the trace kernel
// uses.  All I/O is in 8-byte slots: doubles for real values (exact for binary32 inputs),
// raw uint64 for RNG state words.  Slot layouts are documented in tests/test_gpu_units.py.
// Ops 32-35 (U_FLUSH_*): the candidate sinks of ops 17-20 with one more raw-uint64 slot per ray, four 16-bit counts of the early resolves of
// a full candidate list during that ray's scan -- bits 0-15 A, 16-31 B, 32-47 C (hit_world_mfma: ops 34, 35), bits 48-63 D (hit_world: op 32)
// or E (hit_world_cull: op 33); the kinds are RTW_FLUSH_* of rtw_scan.hpp.  36 is the first number behind the last op; 24 and 29 are no ops.
#pragma once
#include "rtw_device.hpp"

namespace rtw {

enum UnitOp {
    U_HIT_SPHERE = 0, U_REFLECT = 1, U_REFRACT = 2, U_REFLECTANCE = 3, U_SCATTER = 4,
    U_GET_RAY = 5, U_SKYCOLOR = 6, U_RNG = 7, U_HIT_WORLD = 8, U_RAY_COLOR = 9,
    U_HIT_WORLD_LDS = 10,    // hit_world with the scene staged in LDS (the trace kernel's instantiation)
    U_HIT_WORLD_CULL = 11,   // hit_world_cull (RTW_FLAG_GROUP_CULL), scene staged in LDS
    U_FX_SUM = 12,           // exact 64.64 accumulation of 8 doubles -> rounded sum, poison count
    U_HIT_WORLD_MFMA = 13,   // hit_world_mfma (pass 1 on the matrix pipe), scene staged in LDS; tmin / tmax of ray 0 serve the whole launch
    U_HIT_WORLD_MFMA_CULL = 14,   // hit_world_mfma with block culling (RTW_FLAG_GROUP_CULL on the matrix pipe), cull layout staged in LDS
    U_NEAR_ZERO = 15,        // near_zero(v) (src/vec.jl:20): squared length against the Float64 literal 1e-5
    U_EXACT_MATH = 16,       // t_sqrt / t_rcp against the compiler's IEEE sqrt / division on a RANGE of binary32 bit patterns (Float32 only)
    // pass-1 candidate sinks (and ops 32-35, below: the same with a count of the early resolves): the scans of ops 10, 11, 13, 14 with a CandSink -- per ray what pass 2 was handed instead of the hit (scenes of <= 512 spheres)
    U_SINK_LDS = 17, U_SINK_CULL = 18, U_SINK_MFMA = 19, U_SINK_MFMA_CULL = 20,
    // the accumulator's tile kernels on hand-made words (rtw_accum_kernels.hip accum_unit; whole-call layouts, not per item: include/rtw_hip.h): the
    // stopping rule's two check kernels, the two compactions, the per-tile resolve.  rtw_unit.hip hands them over before its per-item path.
    U_ACCUM_TILE_CHECK = 21, U_ACCUM_COMPACT = 22, U_ACCUM_RESOLVE_TILES = 23,
    // (24 is not an op: callers probe it as the first unknown number)
    U_ACCUM_NOISE = 25,      // the noise map kernel of an adaptive accumulator on hand-made words and C_t (rtw_accum_kernels.hip accum_unit)
    // one bounce as the trace kernel composes it (rtw_kernels.hpp phases H2, R, F): hit_world, then make_hitrec, the DielConst of the uploaded cold
    // rows, scatter_begin(..., &dc), attenuation_of, the rejection loop, scatter_finish, the final normalize
    U_SHADE = 26,
    // op 20's scan with a sink that also records the block vote: RTW_SINK_SLOTS slots as op 20, then one raw uint64 -- bit b: block b of the cull
    // layout's device order was voted for by the half wave of this ray (the first group of 32 blocks: all there is within RTW_SINK_SPHERES)
    U_SINK_MFMA_CULL_VOTE = 27,
    // the cull layout itself: item p is device position p (block p / 32).  out: the caller's index of the sphere there (-1: a dead or padding slot, or
    // p beyond the layout), 1 if that position is in the in-lane list, the number of positions, the number of blocks
    U_CULL_LAYOUT = 28,
    // (29 is not an op either: the first number behind op 28 stays the unknown one callers probe)
    // the batched per-tile resolve and the batched noise map on hand-made words and C_t, N views in ONE launch next to the single kernels view by view (rtw_accum_kernels.hip accum_unit)
    U_ACCUM_RESOLVE_BATCH = 30, U_ACCUM_NOISE_BATCH = 31,
    // the sinks of ops 17-20 with a flush counter: RTW_SINK_SLOTS slots as there, then one raw uint64 of four 16-bit counts -- how often a full candidate
    // list was resolved early during this ray's scan (NoSink::flush, rtw_scan.hpp), field RTW_FLUSH_*: bits 0-15 A, 16-31 B, 32-47 C (ops 34, 35), bits
    // 48-63 D (op 32) or E (op 33).  A - D are the wave's and stand in every live row alike; E is the lane's own.
    U_FLUSH_LDS = 32, U_FLUSH_CULL = 33, U_FLUSH_MFMA = 34, U_FLUSH_MFMA_CULL = 35,
    U_NUM_OPS = 36
};
__host__ __device__ inline bool unit_is_accum(int op) {
    return (op >= U_ACCUM_TILE_CHECK && op <= U_ACCUM_RESOLVE_TILES) || op == U_ACCUM_NOISE || op == U_ACCUM_RESOLVE_BATCH || op == U_ACCUM_NOISE_BATCH;
}
__host__ __device__ inline bool unit_is_flush(int op) { return op >= U_FLUSH_LDS && op <= U_FLUSH_MFMA_CULL; }
__host__ __device__ inline bool unit_is_sink(int op) { return (op >= U_SINK_LDS && op <= U_SINK_MFMA_CULL) || op == U_SINK_MFMA_CULL_VOTE || unit_is_flush(op); }
__host__ __device__ inline int unit_sink_of(int op) { return unit_is_flush(op) ? op - U_FLUSH_LDS + U_SINK_LDS : op; }      // the sink op whose scan a flush op runs
#define RTW_SINK_SPHERES 512
#define RTW_SINK_SLOTS 18
#define RTW_VOTE_SLOTS (RTW_SINK_SLOTS + 1)
#define RTW_FLUSH_SLOTS (RTW_SINK_SLOTS + 1)

__host__ __device__ inline int unit_in_slots(int op) {
    switch (op) {
        case U_HIT_SPHERE: return 12;   // c[3], r, o[3], d[3], tmin, tmax
        case U_REFLECT: return 6;       // v[3], n[3]
        case U_REFRACT: return 7;       // d[3], n[3], ratio
        case U_REFLECTANCE: return 2;   // cos, ratio
        case U_SCATTER: return 18;      // state[2], kind, albedo[3], param, d[3], rec{t,p[3],n[3],front}
        case U_GET_RAY: return 4;       // state[2], s, t
        case U_SKYCOLOR: return 3;      // d[3]
        case U_RNG: return 2;           // state[2]
        case U_NEAR_ZERO: return 3;     // v[3]
        case U_EXACT_MATH: return 2;    // first bit pattern, number of consecutive patterns
        case U_HIT_WORLD: case U_HIT_WORLD_LDS: case U_HIT_WORLD_CULL: case U_HIT_WORLD_MFMA: case U_HIT_WORLD_MFMA_CULL: return 8;     // o[3], d[3], tmin, tmax
        case U_SINK_LDS: case U_SINK_CULL: case U_SINK_MFMA: case U_SINK_MFMA_CULL: case U_SINK_MFMA_CULL_VOTE: return 8;             // (the same)
        case U_FLUSH_LDS: case U_FLUSH_CULL: case U_FLUSH_MFMA: case U_FLUSH_MFMA_CULL: return 8;                                    // (the same)
        case U_CULL_LAYOUT: return 1;   // (ignored)
        case U_RAY_COLOR: return 9;     // state[2], o[3], d[3], depth
        case U_FX_SUM: return 8;        // 8 binary64 values
        case U_SHADE: return 8;         // state[2], o[3], d[3]
    }
    return 0;
}
__host__ __device__ inline int unit_out_slots(int op) {
    switch (op) {
        case U_HIT_SPHERE: return 9;    // hit, t, p[3], n[3], front
        case U_REFLECT: return 3;
        case U_REFRACT: return 3;
        case U_REFLECTANCE: return 1;
        case U_SCATTER: return 11;      // state[2], o[3], d[3], att[3]
        case U_GET_RAY: return 8;       // state[2], o[3], d[3]
        case U_SKYCOLOR: return 3;
        case U_RNG: return 6;           // state[2], 4 uniforms
        case U_NEAR_ZERO: return 2;     // near_zero(v), squared_length(v) (src/vec.jl:19-20)
        case U_EXACT_MATH: return 4;    // mismatches of t_sqrt, of t_rcp, first bad pattern of each (or -1)
        case U_HIT_WORLD: case U_HIT_WORLD_LDS: case U_HIT_WORLD_CULL: case U_HIT_WORLD_MFMA: case U_HIT_WORLD_MFMA_CULL: return 9;     // idx, t, p[3], n[3], front
        case U_SINK_LDS: case U_SINK_CULL: case U_SINK_MFMA: case U_SINK_MFMA_CULL: return RTW_SINK_SLOTS;   // ok, mf_sc, cand bits[8], in-lane bits[8] (raw uint64)
        case U_SINK_MFMA_CULL_VOTE: return RTW_VOTE_SLOTS;   // op 20's slots, voted blocks (raw uint64)
        case U_FLUSH_LDS: case U_FLUSH_CULL: case U_FLUSH_MFMA: case U_FLUSH_MFMA_CULL: return RTW_FLUSH_SLOTS;   // the sink's slots, early resolves (raw uint64: 4 x 16 bits)
        case U_CULL_LAYOUT: return 4;   // the caller's index or -1, in-lane, positions, blocks
        case U_RAY_COLOR: return 6;     // state[2], colour[3], segments
        case U_FX_SUM: return 2;        // sum, poisoned
        case U_SHADE: return 12;        // state[2], idx, o[3], d[3], att[3] (a miss: the state as it came, idx = -1, zeros)
    }
    return 0;
}

template <typename T>
__device__ __forceinline__ V3<T> ld3(const double *p) { return {(T)p[0], (T)p[1], (T)p[2]}; }
template <typename T>
__device__ __forceinline__ void st3(double *p, V3<T> v) { p[0] = (double)v.x; p[1] = (double)v.y; p[2] = (double)v.z; }
__device__ __forceinline__ uint64_t as_u64(double d) { return (uint64_t)__double_as_longlong(d); }
__device__ __forceinline__ double as_f64(uint64_t u) { return __longlong_as_double((long long)u); }

// The sink of ops 17-20 (rtw_scan.hpp NoSink): rows of RTW_SINK_SLOTS 8-byte slots, one per ray of the wave, zeroed by the host.  Bit i & 63 of
// slot 2 + (i >> 6) / 10 + (i >> 6): sphere i of the caller's list.  A row belongs to the lane's ray but any lane may record into it (hit_world_mfma:
// the lane that runs a candidate's exact test is not its owner): global atomic ORs.
// Op 27 (SLOTS = RTW_VOTE_SLOTS): the same rows with one more slot, the blocks the ray's half wave voted for (blocks(): every lane records into its
// OWN row what its half of the wave-uniform vote words says).
// Ops 32-35 (SLOTS = RTW_FLUSH_SLOTS, FLUSH_SLOT = RTW_SINK_SLOTS): the same rows with one more slot, four 16-bit counts of early resolves (flush():
// the lane adds 1 to field `kind` of its OWN row; the other sinks count nothing).
template <int SLOTS, int FLUSH_SLOT = -1>
struct CandSinkT {
    double *rows;          // the wave's first row
    unsigned n_live;       // rows of the wave (lanes beyond have no ray and no row)
    unsigned self;         // this lane
    static constexpr bool on() { return true; }
    __device__ void ray(unsigned lane, bool ok, float sc) {
        if (lane < n_live) { rows[lane * SLOTS] = ok ? 1.0 : 0.0; rows[lane * SLOTS + 1] = (double)sc; }
    }
    __device__ void bit(unsigned lane, int slot0, int i) {
        if (lane < n_live && (unsigned)i < (unsigned)RTW_SINK_SPHERES)
            atomicOr(reinterpret_cast<unsigned long long *>(rows + lane * SLOTS + slot0 + (i >> 6)), 1ull << (i & 63));
    }
    __device__ void cand(unsigned lane, int i) { bit(lane, 2, i); }
    __device__ void inlane(unsigned lane, int i) { bit(lane, 10, i); }
    __device__ void blocks(unsigned lane, int base, unsigned v0, unsigned v1) {
        if constexpr (SLOTS > RTW_SINK_SLOTS && FLUSH_SLOT < 0) {
            if (lane < n_live && (unsigned)base < 64u)
                atomicOr(reinterpret_cast<unsigned long long *>(rows + lane * SLOTS + RTW_SINK_SLOTS), (unsigned long long)(lane < 32u ? v0 : v1) << base);
        }
    }
    __device__ void flush(unsigned lane, int kind) {
        if constexpr (FLUSH_SLOT >= 0) {
            if (lane < n_live) atomicAdd(reinterpret_cast<unsigned long long *>(rows + lane * SLOTS + FLUSH_SLOT), 1ull << (16 * kind));
        }
    }
};
using CandSink = CandSinkT<RTW_SINK_SLOTS>;
using VoteSink = CandSinkT<RTW_VOTE_SLOTS>;
using FlushSink = CandSinkT<RTW_FLUSH_SLOTS, RTW_SINK_SLOTS>;

template <typename T>
__global__ void unit_kernel(int op, int count, const double *__restrict__ in, double *__restrict__ out,
                            DevScene<T> scene, CullScene<T> cull, Camera<T> cam) {
    using V4 = typename Vec4<T>::type;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    __shared__ unsigned short s_list[RTW_LIST_CAP * 64];    // launched with 64-thread blocks
    extern __shared__ __attribute__((aligned(16))) unsigned char u_smem[];   // ops 10, 11: the staged scene
    unsigned short *my_list = s_list + threadIdx.x;
    const bool live = gid < count;                          // no early return: the scan is wave-cooperative
    const double *x = in + (size_t)gid * unit_in_slots(op);
    double *y = out + (size_t)gid * unit_out_slots(op);
    const bool coop = op == U_HIT_WORLD || op == U_RAY_COLOR || op == U_HIT_WORLD_LDS || op == U_HIT_WORLD_CULL || op == U_HIT_WORLD_MFMA || op == U_HIT_WORLD_MFMA_CULL || op == U_SHADE || unit_is_sink(op);
    const int wave0 = gid - (int)(threadIdx.x & 63u);
    const CandSink sink = {out + (size_t)wave0 * RTW_SINK_SLOTS, (unsigned)(count - wave0 < 64 ? count - wave0 : 64), threadIdx.x & 63u};   // (ops 17-20)
    const VoteSink vsink = {out + (size_t)wave0 * RTW_VOTE_SLOTS, sink.n_live, sink.self};                                                   // (op 27)
    const FlushSink fsink = {out + (size_t)wave0 * RTW_FLUSH_SLOTS, sink.n_live, sink.self};                                                 // (ops 32-35)
    if (!coop && !live) return;
    switch (op) {
        case U_HIT_SPHERE: {
            V3<T> c = ld3<T>(x), o = ld3<T>(x + 4), d = ld3<T>(x + 7);
            T r = (T)x[3], tmin = (T)x[10], tmax = (T)x[11];
            T hb, disc, root;
            sphere_disc<T>(scene.numerics, c.x, c.y, c.z, r * r, r, o, d, hb, disc);
            for (int k = 0; k < 9; ++k) y[k] = 0.0;
            if (sphere_root<T>(hb, disc, tmin, tmax, root)) {
                HitRec<T> rec;
                make_hitrec<T>(c, r, o, d, root, rec);
                y[0] = 1.0; y[1] = (double)rec.t; st3(y + 2, rec.p); st3(y + 5, rec.n); y[8] = rec.front ? 1.0 : 0.0;
            }
        } break;
        case U_REFLECT: st3(y, reflect(ld3<T>(x), ld3<T>(x + 3))); break;
        case U_REFRACT: st3(y, refract(ld3<T>(x), ld3<T>(x + 3), (T)x[6])); break;
        case U_REFLECTANCE: y[0] = (double)reflectance((T)x[0], (T)x[1]); break;
        case U_SCATTER: {
            Rng rng = {as_u64(x[0]), as_u64(x[1])};
            HitRec<T> rec;
            rec.t = (T)x[10]; rec.p = ld3<T>(x + 11); rec.n = ld3<T>(x + 14); rec.front = x[17] != 0.0;
            V3<T> nd, att;
            scatter<T>(rng, (int)x[2], ld3<T>(x + 3), (T)x[6], ld3<T>(x + 7), rec, nd, att);
            y[0] = as_f64(rng.x); y[1] = as_f64(rng.y);
            st3(y + 2, rec.p); st3(y + 5, nd); st3(y + 8, att);
        } break;
        case U_GET_RAY: {
            Rng rng = {as_u64(x[0]), as_u64(x[1])};
            V3<T> o, d;
            get_ray(rng, cam, (T)x[2], (T)x[3], o, d);
            y[0] = as_f64(rng.x); y[1] = as_f64(rng.y);
            st3(y + 2, o); st3(y + 5, d);
        } break;
        case U_SKYCOLOR: {
            C3 c = skycolor(ld3<T>(x));
            y[0] = c.r; y[1] = c.g; y[2] = c.b;
        } break;
        case U_RNG: {
            Rng rng = {as_u64(x[0]), as_u64(x[1])};
            for (int k = 0; k < 4; ++k) { T u; trand(rng, u); y[2 + k] = (double)u; }
            y[0] = as_f64(rng.x); y[1] = as_f64(rng.y);
        } break;
        case U_EXACT_MATH: {
            // (the waves of this launch see consecutive patterns in their lanes: in-range and out-of-range arguments mix, as in the kernel)
            double bad_s = 0, bad_r = 0, first_s = -1, first_r = -1;
            if constexpr (sizeof(T) == 4) {
                const unsigned p0 = (unsigned)x[0], n = (unsigned)x[1];
                for (unsigned k = 0; k < n; ++k) {
                    const unsigned u = p0 + k;
                    const float v = __uint_as_float(u);
                    const unsigned a = __float_as_uint(t_sqrt(v)), b = __float_as_uint(__builtin_sqrtf(v));
                    const unsigned c = __float_as_uint(t_rcp(v)), e = __float_as_uint(1.0f / v);
                    const bool nan_ab = (a & 0x7fffffffu) > 0x7f800000u && (b & 0x7fffffffu) > 0x7f800000u;      // (any NaN equals any NaN)
                    const bool nan_ce = (c & 0x7fffffffu) > 0x7f800000u && (e & 0x7fffffffu) > 0x7f800000u;
                    if (a != b && !nan_ab) { bad_s += 1; if (first_s < 0) first_s = (double)u; }
                    if (c != e && !nan_ce) { bad_r += 1; if (first_r < 0) first_r = (double)u; }
                }
            }
            y[0] = bad_s; y[1] = bad_r; y[2] = first_s; y[3] = first_r;
        } break;
        case U_NEAR_ZERO: {
            const V3<T> v = ld3<T>(x);
            y[0] = near_zero(v) ? 1.0 : 0.0;
            y[1] = (double)dot(v, v);
        } break;
        case U_HIT_WORLD: {
            V3<T> o = {0, 0, 0}, d = {0, 0, 1};
            T tmn = 0, tmx = 0;
            if (live) { o = ld3<T>(x); d = ld3<T>(x + 3); tmn = (T)x[6]; tmx = (T)x[7]; }
            T t_hit;
            int idx = hit_world<T, 64>(scene, scene.geom, o, d, tmn, tmx, t_hit, my_list);
            if (!live) return;
            for (int k = 0; k < 9; ++k) y[k] = 0.0;
            y[0] = (double)idx;
            if (idx >= 0) {
                auto g = scene.geom[idx];
                auto m0 = scene.mat0[idx];
                HitRec<T> rec;
                make_hitrec<T>({g.x, g.y, g.z}, m0.x, o, d, t_hit, rec);
                y[1] = (double)rec.t; st3(y + 2, rec.p); st3(y + 5, rec.n); y[8] = rec.front ? 1.0 : 0.0;
            }
        } break;
        case U_HIT_WORLD_LDS: case U_HIT_WORLD_CULL: {
            V4 *lds_geom = reinterpret_cast<V4 *>(u_smem);
            unsigned short *lds_orig = reinterpret_cast<unsigned short *>(lds_geom + (op == U_HIT_WORLD_CULL ? cull_exact_count(cull) : 0));
            if (op == U_HIT_WORLD_CULL) stage_cull_scene<T>(cull, lds_geom, lds_orig); else stage_scene<T>(scene, lds_geom);
            __syncthreads();
            V3<T> o = {0, 0, 0}, d = {0, 0, 1};
            T tmn = 0, tmx = 0;
            if (live) { o = ld3<T>(x); d = ld3<T>(x + 3); tmn = (T)x[6]; tmx = (T)x[7]; }
            T t_hit;
            int idx;
            if (op == U_HIT_WORLD_CULL)
                idx = hit_world_cull<T, 64>(cull, (const V4 *)lds_geom, (const unsigned short *)lds_orig, o, d, tmn, tmx, t_hit, my_list);
            else
                idx = hit_world<T, 64>(scene, (const V4 *)lds_geom, o, d, tmn, tmx, t_hit, my_list);
            if (!live) return;
            for (int k = 0; k < 9; ++k) y[k] = 0.0;
            y[0] = (double)(idx >= 0 && op == U_HIT_WORLD_CULL ? (int)cull.orig[idx] : idx);   // index in the caller's list
            if (idx >= 0) {
                const V4 g = op == U_HIT_WORLD_CULL ? cull.exact[idx] : scene.geom[idx];
                const V4 m0 = op == U_HIT_WORLD_CULL ? cull.mat0[idx] : scene.mat0[idx];
                HitRec<T> rec;
                make_hitrec<T>({g.x, g.y, g.z}, m0.x, o, d, t_hit, rec);
                y[1] = (double)rec.t; st3(y + 2, rec.p); st3(y + 5, rec.n); y[8] = rec.front ? 1.0 : 0.0;
            }
        } break;
        case U_HIT_WORLD_MFMA: {
            __shared__ __attribute__((aligned(8))) unsigned s_pairs[RTW_PAIR_CAP];
            __shared__ unsigned long long s_keys[64];
            __shared__ unsigned s_kidx[64];
            V4 *lds_geom = reinterpret_cast<V4 *>(u_smem);
            stage_scene<T>(scene, lds_geom);
            __syncthreads();
            V3<T> o = {0, 0, 0}, d = {0, 0, 1};
            if (live) { o = ld3<T>(x); d = ld3<T>(x + 3); }
            const T tmn = (T)in[6];                       // wave-uniform by contract (the trace kernel passes a constant)
            T t_hit;
            const WaveScratch ws = {s_pairs, s_keys, s_kidx};
            int idx = -1;
            if (scene.mf_ops) idx = hit_world_mfma<T>(scene, (const V4 *)lds_geom, o, d, live, tmn, t_hit, ws, threadIdx.x & 63u);
            if (!live) return;
            for (int k = 0; k < 9; ++k) y[k] = 0.0;
            y[0] = (double)idx;
            if (idx >= 0) {
                const V4 g = scene.geom[idx];
                const V4 m0 = scene.mat0[idx];
                HitRec<T> rec;
                make_hitrec<T>({g.x, g.y, g.z}, m0.x, o, d, t_hit, rec);
                y[1] = (double)rec.t; st3(y + 2, rec.p); st3(y + 5, rec.n); y[8] = rec.front ? 1.0 : 0.0;
            }
        } break;
        case U_HIT_WORLD_MFMA_CULL: {
            __shared__ __attribute__((aligned(8))) unsigned c_pairs[RTW_PAIR_CAP];
            __shared__ unsigned long long c_keys[64];
            __shared__ unsigned c_kidx[64];
            V4 *lds_geom = reinterpret_cast<V4 *>(u_smem);
            unsigned short *lds_orig = reinterpret_cast<unsigned short *>(lds_geom + cull_exact_count(cull));
            stage_cull_scene<T>(cull, lds_geom, lds_orig);
            __syncthreads();
            V3<T> o = {0, 0, 0}, d = {0, 0, 1};
            if (live) { o = ld3<T>(x); d = ld3<T>(x + 3); }
            const T tmn = (T)in[6];
            T t_hit;
            const WaveScratch ws = {c_pairs, c_keys, c_kidx};
            const MfmaCull mc = mfma_cull_of(cull);
            int idx = -1;
            if (cull.mf_ops) idx = hit_world_mfma<T>(scene, (const V4 *)lds_geom, o, d, live, tmn, t_hit, ws, threadIdx.x & 63u, NoClock(), &mc, (const unsigned short *)lds_orig);
            if (!live) return;
            for (int k = 0; k < 9; ++k) y[k] = 0.0;
            y[0] = (double)(idx >= 0 ? (int)cull.orig[idx] : idx);      // index in the caller's list
            if (idx >= 0) {
                const V4 g = cull.exact[idx];
                const V4 m0 = cull.mat0[idx];
                HitRec<T> rec;
                make_hitrec<T>({g.x, g.y, g.z}, m0.x, o, d, t_hit, rec);
                y[1] = (double)rec.t; st3(y + 2, rec.p); st3(y + 5, rec.n); y[8] = rec.front ? 1.0 : 0.0;
            }
        } break;
        case U_SINK_LDS: case U_SINK_CULL: case U_FLUSH_LDS: case U_FLUSH_CULL: {
            V4 *lds_geom = reinterpret_cast<V4 *>(u_smem);
            const bool culled = unit_sink_of(op) == U_SINK_CULL;
            unsigned short *lds_orig = reinterpret_cast<unsigned short *>(lds_geom + (culled ? cull_exact_count(cull) : 0));
            if (culled) stage_cull_scene<T>(cull, lds_geom, lds_orig); else stage_scene<T>(scene, lds_geom);
            __syncthreads();
            V3<T> o = {0, 0, 0}, d = {0, 0, 1};
            T tmn = 0, tmx = 0;
            if (live) { o = ld3<T>(x); d = ld3<T>(x + 3); tmn = (T)x[6]; tmx = (T)x[7]; }
            T t_hit;
            if (op == U_FLUSH_CULL)
                hit_world_cull<T, 64>(cull, (const V4 *)lds_geom, (const unsigned short *)lds_orig, o, d, tmn, tmx, t_hit, my_list, NoClock(), fsink);
            else if (op == U_FLUSH_LDS)
                hit_world<T, 64>(scene, (const V4 *)lds_geom, o, d, tmn, tmx, t_hit, my_list, NoClock(), fsink);
            else if (op == U_SINK_CULL)
                hit_world_cull<T, 64>(cull, (const V4 *)lds_geom, (const unsigned short *)lds_orig, o, d, tmn, tmx, t_hit, my_list, NoClock(), sink);
            else
                hit_world<T, 64>(scene, (const V4 *)lds_geom, o, d, tmn, tmx, t_hit, my_list, NoClock(), sink);
        } break;
        case U_SINK_MFMA: case U_SINK_MFMA_CULL: case U_SINK_MFMA_CULL_VOTE: case U_FLUSH_MFMA: case U_FLUSH_MFMA_CULL: {
            __shared__ __attribute__((aligned(8))) unsigned k_pairs[RTW_PAIR_CAP];
            __shared__ unsigned long long k_keys[64];
            __shared__ unsigned k_kidx[64];
            V4 *lds_geom = reinterpret_cast<V4 *>(u_smem);
            const bool culled = unit_sink_of(op) != U_SINK_MFMA;
            unsigned short *lds_orig = reinterpret_cast<unsigned short *>(lds_geom + (culled ? cull_exact_count(cull) : 0));
            if (culled) stage_cull_scene<T>(cull, lds_geom, lds_orig); else stage_scene<T>(scene, lds_geom);
            __syncthreads();
            V3<T> o = {0, 0, 0}, d = {0, 0, 1};
            if (live) { o = ld3<T>(x); d = ld3<T>(x + 3); }
            const T tmn = (T)in[6];
            T t_hit;
            const WaveScratch ws = {k_pairs, k_keys, k_kidx};
            if (op == U_FLUSH_MFMA_CULL) {
                const MfmaCull mc = mfma_cull_of(cull);
                hit_world_mfma<T>(scene, (const V4 *)lds_geom, o, d, live, tmn, t_hit, ws, threadIdx.x & 63u, NoClock(), &mc, (const unsigned short *)lds_orig, fsink);
            } else if (op == U_FLUSH_MFMA) {
                hit_world_mfma<T>(scene, (const V4 *)lds_geom, o, d, live, tmn, t_hit, ws, threadIdx.x & 63u, NoClock(), nullptr, NoOrig(), fsink);
            } else if (op == U_SINK_MFMA_CULL_VOTE) {
                const MfmaCull mc = mfma_cull_of(cull);
                hit_world_mfma<T>(scene, (const V4 *)lds_geom, o, d, live, tmn, t_hit, ws, threadIdx.x & 63u, NoClock(), &mc, (const unsigned short *)lds_orig, vsink);
            } else if (op == U_SINK_MFMA_CULL) {
                const MfmaCull mc = mfma_cull_of(cull);
                hit_world_mfma<T>(scene, (const V4 *)lds_geom, o, d, live, tmn, t_hit, ws, threadIdx.x & 63u, NoClock(), &mc, (const unsigned short *)lds_orig, sink);
            } else {
                hit_world_mfma<T>(scene, (const V4 *)lds_geom, o, d, live, tmn, t_hit, ws, threadIdx.x & 63u, NoClock(), nullptr, NoOrig(), sink);
            }
        } break;
        case U_CULL_LAYOUT: {
            // (the host refuses a scene without matrix-pipe cull operands: the tables, with the in-lane list, lie behind the block boxes)
            const int n_pos = cull_exact_count(cull);
            const MfmaCull mc = mfma_cull_of(cull);
            int idx = -1;
            bool inl = false;
            if (gid < n_pos && !((double)cull.exact[gid].w < -1e29)) {
                idx = (int)cull.orig[gid];
                for (int k = 0; k < mc.n_huge && k < RTW_CULL_INLANE_MAX; ++k) inl = inl || (int)mc.tab[6 * RTW_CULL_BINS + 4 + k] == gid;
            }
            y[0] = (double)idx; y[1] = inl ? 1.0 : 0.0; y[2] = (double)n_pos; y[3] = (double)mc.blocks;
        } break;
        case U_FX_SUM: {
            // the trace kernel's pixel accumulation: fx_from_double -> 128-bit adds -> fx_to_double
            unsigned long long lo = 0, hi = 0, bad = 0;
            for (int k = 0; k < 8; ++k) {
                unsigned long long l, h;
                if (fx_from_double(x[k], l, h)) { const unsigned long long old = lo; lo += l; hi += h + (lo < old ? 1ull : 0ull); }
                else bad += 1;
            }
            y[0] = bad ? __builtin_nan("") : fx_to_double(lo, hi);
            y[1] = (double)bad;
        } break;
        case U_RAY_COLOR: {
            // src/ray_color.jl:14-38 as the iterative front-to-back loop of the trace kernel
            Rng rng = {1, 2};
            V3<T> o = {0, 0, 0}, d = {0, 0, 1};
            int depth = 0;
            if (live) { rng = {as_u64(x[0]), as_u64(x[1])}; o = ld3<T>(x + 2); d = ld3<T>(x + 5); depth = (int)x[8]; }
            double tr = 1, tg = 1, tb = 1, cr = 0, cg = 0, cb = 0;
            unsigned segs = 0;
            bool active = depth > 0;
            while (__any(active)) {                   // the scan is wave-cooperative: all lanes enter it
                T t_hit;
                int idx = hit_world<T, 64>(scene, scene.geom, o, d, (T)1e-4, (T)__builtin_huge_val(), t_hit, my_list);
                if (!active) continue;
                segs++;
                if (idx < 0) {
                    C3 sky = skycolor(d);
                    cr = tr * sky.r; cg = tg * sky.g; cb = tb * sky.b;
                    active = false;
                    continue;
                }
                auto g = scene.geom[idx];
                auto m0 = scene.mat0[idx];
                auto m1 = scene.mat1[idx];
                HitRec<T> rec;
                make_hitrec<T>({g.x, g.y, g.z}, m0.x, o, d, t_hit, rec);
                V3<T> nd, att;
                scatter<T>(rng, (int)m0.z, {m1.x, m1.y, m1.z}, m0.y, d, rec, nd, att);
                tr = tr * (double)att.x; tg = tg * (double)att.y; tb = tb * (double)att.z;
                o = rec.p; d = nd;
                depth -= 1;
                if (depth <= 0) active = false;
            }
            if (!live) return;
            y[0] = as_f64(rng.x); y[1] = as_f64(rng.y);
            y[2] = cr; y[3] = cg; y[4] = cb; y[5] = (double)segs;
        } break;
        case U_SHADE: {
            // rtw_kernels.hpp phases H2, R, F for one segment: the calls and their order are the trace kernel's, on the rows the upload made
            Rng rng = {1, 2};
            V3<T> o = {0, 0, 0}, d = {0, 0, 1};
            if (live) { rng = {as_u64(x[0]), as_u64(x[1])}; o = ld3<T>(x + 2); d = ld3<T>(x + 5); }
            T t_hit;
            const int idx = hit_world<T, 64>(scene, scene.geom, o, d, (T)1e-4, (T)__builtin_huge_val(), t_hit, my_list);
            if (!live) return;
            for (int k = 0; k < 12; ++k) y[k] = 0.0;
            y[2] = (double)idx;
            if (idx >= 0) {
                const V4 g = scene.geom[idx];
                const V4 m0 = scene.mat0[idx];
                const V4 m1 = scene.mat1[idx];
                HitRec<T> rec;
                make_hitrec<T>({g.x, g.y, g.z}, m0.x, o, d, t_hit, rec);
                const int kind = (int)m0.z;
                const DielConst<T> dc = {m0.w, m1.x, m1.y};
                V3<T> vec = {0, 0, 0};
                T vs = 1;
                int todo = scatter_begin<T>(rng, kind, m0.y, d, rec, vec, vs, &dc);
                const V3<T> att = attenuation_of<T>(kind, {m1.x, m1.y, m1.z});
                if (todo == PATH_BALL) {
                    V3<T> rp = {0, 0, 0};
                    T len2 = 0;
                    bool pending = true;
                    while (pending) {
                        len2 = reject_trial<T>(rng, true, rp);
                        pending = !(len2 <= T(1));
                    }
                    todo = scatter_finish<T>(kind, vec, vs, rp, len2, vec);
                }
                if (todo == PATH_NORM) vec = normalize(vec);
                st3(y + 3, rec.p); st3(y + 6, vec); st3(y + 9, att);
            }
            y[0] = as_f64(rng.x); y[1] = as_f64(rng.y);
        } break;
    }
}

}  // namespace rtw
