// rtw_trace_rays.hpp -- the radiance-query kernel: ray_color of caller-supplied rays (include/rtw_hip.h rtw_trace_rays_*).
// gfx950 only; wave = 64 lanes.
//
// The rays are those of the ray-query kernel (rtw_rays.hpp: 8 elements each, elements 6 and 7 not read) and the start is that kernel's: a
// workgroup of RTW_RAYS_WAVES waves, the scene (and the plain scan's index array) staged ONCE, no workgroup barrier behind that, the same
// LDS layout.  Sample s of ray i is src/ray_color.jl:14-38 with the product formed front to back on a fresh stream
// rng_stream(seed, first_stream + i, first_sample + s): one stream per SAMPLE, so the words depend on nothing of the scheduling below.
//
// The lane loop.  Path lengths run from 1 to max_depth, so a wave does not wait for its longest path; per iteration:
//   (S) ONE scan (hit_world_mfma, wave-cooperative, or hit_world) over the lanes that have a ray;
//   (H) a miss adds thr * sky EXACTLY to the lane's three 128-bit sums (registers: the lane owns its ray for all spp samples, so colour needs
//       no LDS and no atomics); a hit scatters -- scatter_begin / reject_trial / scatter_finish / normalize on the dielectric constants the
//       upload stored, as the trace kernel composes them (unit op U_SHADE, tests/test_gpu_material_sweep.py) -- and uses one bounce;
//   (E) a lane whose path ended starts its ray's next sample in the same iteration (fresh stream, thr = 1), or, behind the last sample,
//       resolves its sums (one rounding, the poison rule, / spp) and stores 24 bytes;
//   (A) the idle lanes take the next unassigned rays of the wave's current batch: a ballot of the idle lanes, a prefix rank, a
//       wave-uniform cursor.  A batch that is used up is followed by the next one the wave CLAIMS from a global counter (one atomic per 64
//       rays, DevCounters::next_job[0], zeroed with the record): a static grid stride would fix each wave's share of the list in advance,
//       and a caller's list is not a frame -- a run of rays inside a glass sphere (50 bounces each) among primary misses (1 scan) lands on
//       whichever waves the stride names, and those then run alone at the end.
//   A wave leaves when the counter is past the last batch and no lane has a ray.
#pragma once
#include "rtw_rays.hpp"

namespace rtw {

struct TraceRaysParams {
    unsigned n;                       // rays (< 2^31)
    unsigned n_batches;               // ceil(n / 64)
    int spp, max_depth;
    unsigned long long seed, first_stream, first_sample;
};

// waves per SIMD the kernel is compiled for: the scan's registers, a path, the ray it restarts from and three 128-bit sums
// (profiles/trace_rays_kernel_resources.txt)
template <typename T> struct TraceRaysWaves { static constexpr int value = 4; };
template <> struct TraceRaysWaves<double> { static constexpr int value = 3; };

// MFMA / LDS_SCENE: as cast_rays_kernel.  out: n x 3 binary64.
template <typename T, bool MFMA, bool LDS_SCENE>
__global__ __launch_bounds__(64 * RTW_RAYS_WAVES, (TraceRaysWaves<T>::value)) void trace_rays_kernel(TraceRaysParams P, DevScene<T> scene, const T *__restrict__ rays,
                                                                                                    double *__restrict__ out, DevCounters *ctr) {
    using V4 = typename Vec4<T>::type;
    const unsigned lane = lane_id(), wv = threadIdx.x >> 6;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    [[maybe_unused]] unsigned short *my_list = reinterpret_cast<unsigned short *>(smem) + threadIdx.x;
    unsigned char *cells = smem + rays_list_bytes();
    V4 *lds_geom = reinterpret_cast<V4 *>(smem + rays_fixed_lds_bytes());
    [[maybe_unused]] unsigned short *lds_orig = reinterpret_cast<unsigned short *>(lds_geom + scene_geom_alloc(scene.n, scene.n_pad));
    [[maybe_unused]] WaveScratch ws = {nullptr, nullptr, nullptr};
    if constexpr (MFMA) {
        ws.pairs = reinterpret_cast<unsigned *>(smem) + wv * RTW_PAIR_CAP;
        ws.keys = reinterpret_cast<unsigned long long *>(cells) + wv * 64;
        ws.kidx = reinterpret_cast<unsigned *>(cells + RTW_RAYS_WAVES * 64 * sizeof(unsigned long long)) + wv * 64;
    }
    if constexpr (LDS_SCENE) {
        stage_scene<T>(scene, lds_geom);
        if constexpr (MFMA) { for (int i = threadIdx.x; i < scene_geom_alloc(scene.n, scene.n_pad); i += blockDim.x) lds_orig[i] = scene.orig[i]; }
        __syncthreads();
    }
    // (no workgroup barrier from here on)

    // the lane's ray and its path
    bool have = false, has_ray = false;       // owns a ray; its path has a segment to scan
    unsigned ri = 0;                          // the ray's index
    V3<T> o0 = {0, 0, 0}, d0 = {0, 0, 1};     // the ray as given: every sample starts here
    V3<T> ro = {0, 0, 0}, rd = {0, 0, 1};
    int s_done = 0, depth = 0;
    double thr_r = 1, thr_g = 1, thr_b = 1;
    Rng rng = {1, 2};
    unsigned long long sum[6] = {0, 0, 0, 0, 0, 0};      // r.lo r.hi g.lo g.hi b.lo b.hi
    bool poison = false;
    // the wave's batch (wave-uniform)
    unsigned cursor = 0, cursor_end = 0;
    bool exhausted = false;
    unsigned long long n_segments = 0, n_samples = 0;

#pragma unroll 1
    for (;;) {
        // ---- (A) idle lanes take the next unassigned rays ----
#pragma unroll 1
        while (!exhausted) {
            const unsigned long long take_mask = __ballot(!have);
            if (!take_mask) break;
            if (cursor >= cursor_end) {
                unsigned b = 0;
                if (lane == 0) b = atomicAdd(&ctr->next_job[0], 1u);
                b = uniform(b);
                if (b >= P.n_batches) { exhausted = true; break; }
                cursor = b * 64u;                                      // (n < 2^31: no wrap)
                cursor_end = min(P.n, cursor + 64u);
            }
            const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(take_mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)take_mask, 0u));   // takers below this lane
            const unsigned p = cursor + rank;
            if (!have && p < cursor_end) {
                T unused;
                ray_load<T>(rays + (size_t)p * RTW_RAY_ELEMS, o0, d0, unused);
                ri = p; have = true;
                s_done = 0; poison = false;
                for (int k = 0; k < 6; ++k) sum[k] = 0ull;
                rng_stream(P.seed, P.first_stream + (unsigned long long)p, P.first_sample, rng);
                ro = o0; rd = d0; thr_r = thr_g = thr_b = 1.0; depth = P.max_depth;
                has_ray = depth > 0;                                   // depth <= 0: ray_color returns 0 (src/ray_color.jl:15)
                // max_depth 0: every sample is black and draws nothing -- all but the last are done here, (E) resolves the zero sums at once
                if (P.max_depth <= 0) s_done = P.spp - 1;
            }
            if (P.max_depth <= 0) n_samples += (unsigned long long)(unsigned)(P.spp - 1) * (unsigned long long)min((unsigned)__popcll(take_mask), cursor_end - cursor);
            cursor = min(cursor_end, cursor + (unsigned)__popcll(take_mask));
        }
        if (!__any(have)) break;

        // ---- (S) one scan of the lanes that have a ray ----
        T t_hit = 0;
        int idx = -1;
        if constexpr (MFMA) {
            if (__any(has_ray)) {
                if (LDS_SCENE) idx = hit_world_mfma<T, const V4 *, const unsigned short *, NoClock, NoSink, false>(scene, (const V4 *)lds_geom, ro, rd, has_ray, (T)1e-4, t_hit, ws, lane, NoClock(), nullptr, (const unsigned short *)lds_orig);
                else idx = hit_world_mfma<T, const V4 *, const unsigned short *, NoClock, NoSink, false>(scene, scene.geom, ro, rd, has_ray, (T)1e-4, t_hit, ws, lane, NoClock(), nullptr, scene.orig);
            }
        } else if (has_ray) {
            if (LDS_SCENE) idx = hit_world<T, 64 * RTW_RAYS_WAVES>(scene, (const V4 *)lds_geom, ro, rd, (T)1e-4, (T)__builtin_huge_val(), t_hit, my_list);
            else idx = hit_world<T, 64 * RTW_RAYS_WAVES>(scene, scene.geom, ro, rd, (T)1e-4, (T)__builtin_huge_val(), t_hit, my_list);
        }
        n_segments += (unsigned long long)__popcll(__ballot(has_ray));

        // ---- (H) a miss ends the sample with thr * sky; a hit scatters ----
        if (has_ray && idx < 0) {
            const C3 sky = skycolor(rd);
            const double cs[3] = {thr_r * sky.r, thr_g * sky.g, thr_b * sky.b};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                unsigned long long lo, hi;
                if (fx_from_double(cs[c], lo, hi)) {
                    const unsigned long long old = sum[2 * c];
                    sum[2 * c] = old + lo;
                    sum[2 * c + 1] += hi + (sum[2 * c] < old ? 1ull : 0ull);
                } else {
                    poison = true;
                }
            }
            has_ray = false;
        }
        if (has_ray) {
            const V4 g = scene.geom[idx];                 // the scan's own order: what its index refers to
            const V4 m0 = scene.mat0[idx];
            const V4 m1 = scene.mat1[idx];
            HitRec<T> rec;
            make_hitrec<T>({g.x, g.y, g.z}, m0.x, ro, rd, t_hit, rec);
            const int kind = (int)m0.z;
            const DielConst<T> dc = {m0.w, m1.x, m1.y};
            V3<T> vec = {0, 0, 0};
            T vs = 1;
            int todo = scatter_begin<T>(rng, kind, m0.y, rd, rec, vec, vs, &dc);
            const V3<T> att = attenuation_of<T>(kind, {m1.x, m1.y, m1.z});
            thr_r = thr_r * (double)att.x; thr_g = thr_g * (double)att.y; thr_b = thr_b * (double)att.z;
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
            ro = rec.p; rd = vec;
            depth -= 1;
            has_ray = depth > 0;                          // out of depth: the sample adds 0
        }

        // ---- (E) the end of a path: the ray's next sample, or its result ----
        const bool ended = have && !has_ray;
        n_samples += (unsigned long long)__popcll(__ballot(ended));
        if (ended) {
            s_done += 1;
            if (s_done < P.spp) {
                rng_stream(P.seed, P.first_stream + (unsigned long long)ri, P.first_sample + (unsigned long long)(unsigned)s_done, rng);
                ro = o0; rd = d0; thr_r = thr_g = thr_b = 1.0; depth = P.max_depth;
                has_ray = depth > 0;
            } else {
                double *q = out + (size_t)ri * 3u;
                const double n_spp = (double)P.spp;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double v = fx_to_double(sum[2 * c], sum[2 * c + 1]);
                    if (poison) v = __builtin_nan("");
                    q[c] = v / n_spp;
                }
                have = false;
            }
        }
    }
    // what rtw_stats() reports: the samples this wave finished and its scans with a live ray (two adds per wave, at the end of its walk)
    if (lane == 0 && n_samples != 0ull) {
        atomicAdd(&ctr->segments, n_segments);
        atomicAdd(&ctr->samples, n_samples);
    }
}

}  // namespace rtw
