// rtw_features.hpp -- the feature kernel: first-hit albedo, normal, depth and coverage per pixel (include/rtw_hip.h rtw_render_features_*).
// gfx950 only; wave = 64 lanes.
//
// The feature sample of (pixel, chunk c) is the primary ray of the chunk's FIRST sample, built exactly as the trace kernel builds it
// (rtw_kernels.hpp phases B, R, F: the stream of (seed, pixel, c), the jitter iff the sample's global index is not 0, the lens disk) and
// scanned by the trace kernel's own scans; nothing of the path behind the first hit is run.
//
// Work decomposition: ONE plain kernel, no queue, no atomics on the sums, no second kernel.
//   workgroup = RTW_FEATURE_WAVES waves, each wave owns one 8x8 tile (tiles numbered column-major like the image);
//   lane      = pixel (i mod 8) + 8 (j mod 8) of the tile: the primary rays of a wave are neighbours.  The wave walks the chunk range with a
//               wave-uniform trip count; every lane calls the (wave-cooperative) matrix-pipe scan in every iteration, lanes of a ragged
//               tile outside the frame with has_ray = false; no lane leaves before the last scan;
//   sums      = per lane 8 x 128-bit two's-complement integers (64.64 fixed point, fx_from_double) + a poison count, in registers;
//   store     = each lane resolves its 8 slots (sum -> binary64 once -> / chunk_count -> T) and writes them as 16-byte stores.
// Integer sums of per-(pixel, chunk) values: the result does not depend on the scan, the launch shape or anything else but the definition.
#pragma once
#include "rtw_device.hpp"
#include "rtw_kernels.hpp"      // DevCounters, lane_id

namespace rtw {

#define RTW_FEATURE_WAVES 4     // waves = tiles per workgroup

struct FeatParams {
    int width, height;
    int spp, chunk_spp;             // of the whole render
    int chunk_begin, chunk_count;   // this call's range of the render's effective chunks
    int tiles_i;                    // tiles down a column
    unsigned n_tiles;
    uint64_t seed;
};

// LDS of a workgroup: [candidate lists: per-lane lists of the all-VALU scan / per-wave pair lists of the matrix-pipe scan][result cells of the
// matrix-pipe scan: keys, kidx][camera][scene copy + (matrix pipe) its index array: LDS_SCENE only]; every offset a multiple of 16
template <typename T> __host__ __device__ constexpr size_t feat_list_bytes() { return (size_t)RTW_LIST_CAP * 64 * RTW_FEATURE_WAVES * sizeof(unsigned short); }
template <typename T> __host__ __device__ constexpr size_t feat_cell_bytes() { return (size_t)RTW_FEATURE_WAVES * 64 * (sizeof(unsigned long long) + sizeof(unsigned)); }
// (BATCH: one camera per wave -- a workgroup's waves may belong to different views)
template <typename T, bool BATCH = false> __host__ __device__ constexpr size_t feat_cam_bytes() { return (sizeof(Camera<T>) * (BATCH ? RTW_FEATURE_WAVES : 1) + 15) / 16 * 16; }
template <typename T, bool BATCH = false> __host__ __device__ constexpr size_t feat_fixed_lds_bytes() { return feat_list_bytes<T>() + feat_cell_bytes<T>() + feat_cam_bytes<T, BATCH>(); }

// The views of a batched launch (rtw_render_features_batch_*; the BATCH instances): the device arrays upload_views (rtw_launch.hip) fills.
// The batch's tiles are numbered flat, g = v * n_tiles + t, so a workgroup's waves may belong to different views: a frame of one tile
// still fills all RTW_FEATURE_WAVES waves.  View v writes at out + v * view_elems.
template <typename T> struct FeatViews {
    const Camera<T> *cams;              // N cameras
    const unsigned long long *seeds;    // N render seeds
    unsigned total_tiles;               // N * FeatParams::n_tiles (< 2^31)
    unsigned long long view_elems;      // W * H * 8: elements of one view's buffer
};
// ... of a TILED && BATCH launch (rtw_accum_features_batch_* over adaptive accumulators): the same views and, behind them, the device table of
// the N accumulators' tile-chunk arrays (chunks[v][t] = C_t of view v), staged in the buffer the cameras and seeds go up in
template <typename T> struct FeatTiledViews : FeatViews<T> {
    const int *const *chunks;           // N device pointers
};
// the kernel's last argument: the tile-chunk array of the TILED instances (every instance that is not BATCH keeps its signature), the views of a
// BATCH instance, the views and their tile-chunk arrays of a TILED && BATCH one
template <typename T, bool BATCH, bool TILED = false> struct FeatLastArg { using type = const int *__restrict__; };
template <typename T> struct FeatLastArg<T, true, false> { using type = FeatViews<T>; };
template <typename T> struct FeatLastArg<T, true, true> { using type = FeatTiledViews<T>; };

// waves per SIMD the kernel is compiled for: 32 registers of sums next to the scan's own
template <typename T> struct FeatWaves { static constexpr int value = 4; };
template <> struct FeatWaves<double> { static constexpr int value = 3; };

__device__ __forceinline__ void fx_add128(unsigned long long &lo, unsigned long long &hi, unsigned long long l, unsigned long long h) {
    const unsigned long long old = lo;
    lo += l;
    hi += h + (lo < old ? 1ull : 0ull);
}

template <typename T> __device__ __forceinline__ void feat_store8(T *o, const T (&r)[8]);
template <> __device__ __forceinline__ void feat_store8<float>(float *o, const float (&r)[8]) {
    float4 *q = reinterpret_cast<float4 *>(o);
    q[0] = float4{r[0], r[1], r[2], r[3]};
    q[1] = float4{r[4], r[5], r[6], r[7]};
}
template <> __device__ __forceinline__ void feat_store8<double>(double *o, const double (&r)[8]) {
    double2 *q = reinterpret_cast<double2 *>(o);
    q[0] = double2{r[0], r[1]}; q[1] = double2{r[2], r[3]};
    q[2] = double2{r[4], r[5]}; q[3] = double2{r[6], r[7]};
}

// MFMA: hit_world_mfma over the plain scan's own sphere order (scene.orig: ties by the caller's index); otherwise hit_world over the
// caller's order.  Either way `scene`'s geom / mat0 / mat1 are the arrays the scan's index refers to.
// NUMK >= 0: the numerics mode fixed at compile time (the default mode of the headline variant), NUMK < 0: the mode of the arguments.
// TILED: the pass over what an adaptive accumulator holds (rtw_accum_features_*): the wave's tile t gets the chunks [0, C_t) with C_t =
// tile_chunks[t] (the accumulator's device array, >= 1), read once and made wave-uniform; P.chunk_begin / chunk_count are not looked at.
// BATCH: N views in one launch (FeatViews, the last argument): the wave's flat tile g = v * n_tiles + t is tile t of view v, whose camera the
// wave stages in its own LDS cell, whose seed is seeds[v] and whose buffer starts at out + v * view_elems; cam_arg and P.seed are not looked
// at.  Everything behind the tile's coordinates is the code of the other instances.  (The last argument keeps its name `tile_chunks` in
// every form: FeatLastArg says what it is.)
// TILED && BATCH: both -- tile t of view v gets the chunks [0, C) with C = chunks[v][t] of the view's own accumulator, read once and made
// wave-uniform, so the waves of one workgroup may belong to different views AND run different trip counts; like BATCH it has no workgroup
// barrier behind the staging of the scene, and a wave behind the last tile leaves without touching a view.
template <typename T, bool MFMA, bool LDS_SCENE, int NUMK = -1, bool TILED = false, bool BATCH = false>
__global__ __launch_bounds__(64 * RTW_FEATURE_WAVES, (FeatWaves<T>::value)) void features_kernel(FeatParams P, Camera<T> cam_arg, DevScene<T> scene,
                                                                                             T *__restrict__ out, DevCounters *ctr, typename FeatLastArg<T, BATCH, TILED>::type tile_chunks) {
    using V4 = typename Vec4<T>::type;
    if constexpr (NUMK >= 0) scene.numerics = NUMK;
    const unsigned lane = lane_id(), wv = threadIdx.x >> 6;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    [[maybe_unused]] unsigned short *my_list = reinterpret_cast<unsigned short *>(smem) + threadIdx.x;
    unsigned char *cells = smem + feat_list_bytes<T>();
    Camera<T> *sh_cam = reinterpret_cast<Camera<T> *>(cells + feat_cell_bytes<T>());
    V4 *lds_geom = reinterpret_cast<V4 *>(smem + feat_fixed_lds_bytes<T, BATCH>());
    [[maybe_unused]] unsigned short *lds_orig = reinterpret_cast<unsigned short *>(lds_geom + scene_geom_alloc(scene.n, scene.n_pad));
    [[maybe_unused]] WaveScratch ws = {nullptr, nullptr, nullptr};
    if constexpr (MFMA) {
        static_assert(feat_list_bytes<T>() == RTW_FEATURE_WAVES * RTW_PAIR_CAP * sizeof(unsigned), "the pair lists use the per-lane list area");
        ws.pairs = reinterpret_cast<unsigned *>(smem) + wv * RTW_PAIR_CAP;
        ws.keys = reinterpret_cast<unsigned long long *>(cells) + wv * 64;
        ws.kidx = reinterpret_cast<unsigned *>(cells + RTW_FEATURE_WAVES * 64 * sizeof(unsigned long long)) + wv * 64;
    }
    // BATCH: the wave's view and its tile in it, wave-uniform; a wave behind the batch's last tile stages no camera but still helps with the scene
    [[maybe_unused]] unsigned view = 0, tile_b = 0;
    [[maybe_unused]] bool has_tile = true;
    if constexpr (BATCH) {
        const unsigned g = __builtin_amdgcn_readfirstlane(blockIdx.x * RTW_FEATURE_WAVES + wv);
        has_tile = g < tile_chunks.total_tiles;
        view = has_tile ? g / P.n_tiles : 0u;
        tile_b = g - view * P.n_tiles;
        sh_cam += wv;
        if (lane == 0 && has_tile) *sh_cam = tile_chunks.cams[view];
    } else {
        if (threadIdx.x == 0) *sh_cam = cam_arg;
    }
    if constexpr (LDS_SCENE) {
        stage_scene<T>(scene, lds_geom);
        if constexpr (MFMA) { for (int i = threadIdx.x; i < scene_geom_alloc(scene.n, scene.n_pad); i += blockDim.x) lds_orig[i] = scene.orig[i]; }
    }
    __syncthreads();
    // (no workgroup barrier from here on: a wave without a tile may leave)
    unsigned tile;
    [[maybe_unused]] unsigned long long seed = P.seed;
    if constexpr (BATCH) {
        if (!has_tile) return;
        tile = tile_b;
        seed = tile_chunks.seeds[view];
        out += (unsigned long long)view * tile_chunks.view_elems;
    } else {
        tile = blockIdx.x * RTW_FEATURE_WAVES + wv;
        if (tile >= P.n_tiles) return;
    }
    const unsigned tj = tile / (unsigned)P.tiles_i, ti = tile - tj * (unsigned)P.tiles_i;
    const int i0 = (int)(ti * 8u + (lane & 7u)), j0 = (int)(tj * 8u + (lane >> 3));       // 0-based row, column
    const bool valid = i0 < P.height && j0 < P.width;
    const unsigned long long pix = (unsigned long long)j0 * (unsigned)P.height + (unsigned)i0;
    const T w_div = (T)(float)P.width, h_div = (T)(float)P.height;                      // f32_image_width / _height (src/render.jl:16-17)
    const T u0 = (T)((double)(j0 + 1) / (double)P.width);                               // T(j / W),       src/render.jl:26
    const T v0 = (T)((double)(P.height - (i0 + 1)) / (double)P.height);                 // T((H - i) / H), src/render.jl:27

    int chunk_begin = P.chunk_begin, chunk_count = P.chunk_count;
    if constexpr (TILED) {
        chunk_begin = 0;
        if constexpr (BATCH) chunk_count = __builtin_amdgcn_readfirstlane(tile_chunks.chunks[view][tile]);
        else chunk_count = __builtin_amdgcn_readfirstlane(tile_chunks[tile]);
    }

    unsigned long long lo[8] = {0, 0, 0, 0, 0, 0, 0, 0}, hi[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned poison = 0;
    auto add = [&](int k, double v) {
        unsigned long long l, h;
        if (fx_from_double(v, l, h)) fx_add128(lo[k], hi[k], l, h);
        else poison += 1u;
    };
#pragma unroll 1
    for (int c = 0; c < chunk_count; ++c) {
        const unsigned chunk = (unsigned)(chunk_begin + c);
        Rng rng;
        rng_stream(BATCH ? seed : P.seed, pix, chunk, rng);
        T du = 0, dv = 0;
        if ((long long)chunk * P.chunk_spp != 0) {                 // the chunk's first sample is not sample 1 of the pixel (src/render.jl:30-31)
            T r1, r2;
            trand(rng, r1); du = RTW_DIV(r1, w_div);
            trand(rng, r2); dv = RTW_DIV(r2, h_div);
        }
        V3<T> rp = {0, 0, 0};
        T len2;
        do { len2 = reject_trial<T>(rng, false, rp); } while (!(len2 <= T(1)));       // the lens disk (src/rand.jl:31-38)
        V3<T> ro, vec;
        {
            const Camera<T> cam = *sh_cam;
            camera_ray_raw<T>(cam, u0 + du, v0 + dv, rp.x, rp.y, ro, vec);              // src/camera.jl:43-48
        }
        const V3<T> rd = normalize(vec);
        T t_hit = 0;
        int idx = -1;
        if constexpr (MFMA) {
            if (LDS_SCENE) idx = hit_world_mfma<T, const V4 *, const unsigned short *, NoClock, NoSink, false>(scene, (const V4 *)lds_geom, ro, rd, valid, (T)1e-4, t_hit, ws, lane, NoClock(), nullptr, (const unsigned short *)lds_orig);
            else idx = hit_world_mfma<T, const V4 *, const unsigned short *, NoClock, NoSink, false>(scene, scene.geom, ro, rd, valid, (T)1e-4, t_hit, ws, lane, NoClock(), nullptr, scene.orig);
        } else if (valid) {
            if (LDS_SCENE) idx = hit_world<T, 64 * RTW_FEATURE_WAVES>(scene, (const V4 *)lds_geom, ro, rd, (T)1e-4, (T)__builtin_huge_val(), t_hit, my_list);
            else idx = hit_world<T, 64 * RTW_FEATURE_WAVES>(scene, scene.geom, ro, rd, (T)1e-4, (T)__builtin_huge_val(), t_hit, my_list);
        }
        if (valid) {
            if (idx >= 0) {
                const V4 g = scene.geom[idx];         // the scan's own order: what its index refers to
                const V4 m0 = scene.mat0[idx];
                const V4 m1 = scene.mat1[idx];
                HitRec<T> rec;
                make_hitrec<T>({g.x, g.y, g.z}, m0.x, ro, rd, t_hit, rec);
                const V3<T> att = attenuation_of<T>((int)m0.z, {m1.x, m1.y, m1.z});
                add(0, (double)att.x); add(1, (double)att.y); add(2, (double)att.z);
                add(3, (double)rec.n.x); add(4, (double)rec.n.y); add(5, (double)rec.n.z);
                add(6, (double)rec.t);
                hi[7] += 1ull;                                                          // coverage: + 1.0
            } else {
                const C3 sky = skycolor(rd);
                add(0, sky.r); add(1, sky.g); add(2, sky.b);
            }
        }
    }
    if (valid) {
        T r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            double v = fx_to_double(lo[k], hi[k]);
            if (poison != 0u) v = __builtin_nan("");
            r[k] = (T)(v / (double)chunk_count);
        }
        feat_store8<T>(out + pix * 8u, r);
    }
    // what rtw_stats() reports: one scan per pixel inside the frame and chunk (two adds per wave)
    const unsigned long long n = (unsigned long long)__popcll(__ballot(valid)) * (unsigned long long)chunk_count;
    if (lane == 0) {
        atomicAdd(&ctr->segments, n);
        atomicAdd(&ctr->samples, n);
    }
}

}  // namespace rtw
