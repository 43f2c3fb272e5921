/*
 * rtw_hip.h -- C ABI of librtw_hip.so, the MI355X (gfx950) implementation of the hot path
 *              render -> ray_color -> hit/scatter  of claforte/RayTracingWeekend.jl.
 *
 * The reference has NO FFI: its boundary for this path is the exported Julia function
 *     render(scene::HittableList, cam::Camera{T}, image_width=400, n_samples=1) -> Matrix{RGB{T}}
 * (/root/reference/src/render.jl:8-44, export at src/RayTracingWeekend.jl:25).  This header is
 * what a Julia `ccall` shim for that function binds (julia/RTWeekendHIP.jl):
 * plain pointers and sizes only, no torch / HIP types in any signature.
 *
 * Conventions
 *   - every pointer is owned by the caller; the library reads inputs and writes outputs only
 *     during the call and retains nothing (device-side handles excepted, see below);
 *   - return 0 = OK, negative = argument/validation error, positive = hipError_t;
 *     rtw_last_error() returns a thread-local message valid until the next call on that thread;
 *   - never throws, never calls exit/abort;
 *   - there is NO CPU fallback: without a usable HIP device every compute entry point fails.
 */
#ifndef RTW_HIP_H
#define RTW_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTW_ABI_VERSION 4   /* round 6: no field moved; two flags of version 3 are gone from the default library -- RTW_FLAG_NUMERICS_REFERENCE_FMA
                               (64: a numerics mode no compiler was found to emit; the bit is now an unknown flag, -2) and RTW_FLAG_RAY_POOL (8:
                               still defined, but the kernel is a `make POOL=1` build option; the default library answers -7) -- and the default
                               chunk rule of rtw_params.n_chunks changed (below).  Version 3 (round 5): the DEFAULT image became the reference's
                               own un-fused order of hit(::Sphere) (RTW_FLAG_NUMERICS_*; version 2's image = RTW_FLAG_NUMERICS_CONTRACT) and the
                               measurement switches of the environment are honoured only under RTW_ENABLE_TEST_AIDS=1 */

/* Material kinds: Lambertian / Metal / Dielectric (src/material.jl:3-5, 25-29, 37-39). */
enum { RTW_LAMBERTIAN = 0, RTW_METAL = 1, RTW_DIELECTRIC = 2 };

/* A HittableList of Sphere{T} (src/structs.jl:10,31-35) flattened to SoA.  Host pointers. */
typedef struct {
    int32_t n;
    const float *cx, *cy, *cz, *r;   /* Sphere.center, Sphere.radius (may be negative)       */
    const int32_t *kind;             /* RTW_* of Sphere.mat                                  */
    const float *ar, *ag, *ab;       /* albedo (Lambertian, Metal)                           */
    const float *param;              /* Metal.fuzz / Dielectric.ir / 0                       */
} rtw_scene_f32;

typedef struct {
    int32_t n;
    const double *cx, *cy, *cz, *r;
    const int32_t *kind;
    const double *ar, *ag, *ab;
    const double *param;
} rtw_scene_f64;

/* Camera{T}: the 22 scalars in the field order of src/camera.jl:2-9. */
typedef struct {
    float origin[3], lower_left_corner[3], horizontal[3], vertical[3], u[3], v[3], w[3];
    float lens_radius;
} rtw_camera_f32;

typedef struct {
    double origin[3], lower_left_corner[3], horizontal[3], vertical[3], u[3], v[3], w[3];
    double lens_radius;
} rtw_camera_f64;

/* rtw_params.flags.  RTW_FLAG_GROUP_CULL: opt-in accelerated closest-hit scan:
 * spheres are clustered at upload (kd clusters with boxes) and spheres that a ray provably cannot hit are never
 * tested: a block of 32 spatially sorted spheres is visited only when some ray of the half wave can touch its box
 * (default: per-ray block sets looked up from tables, ORed over the half wave),
 * or, with RTW_FLAG_SCAN_VALU, per ray and cluster of 16 on the vector ALUs (the round-1/2 form).
 * Bit-identical images; default (0) is the reference's plain linear scan. */
#define RTW_FLAG_GROUP_CULL 1
/* RTW_FLAG_COMPACT_TILES (device-resident entry points): write only this shard's 8x8 tiles, tile-major
 * and compact -- local tile k (global tile k*shard_count + shard_index, tiles numbered column-major like
 * the image) at [k*64 + (i mod 8) + 8*(j mod 8)]*3 -- instead of the zero-padded full frame: the buffer is
 * ceil((n_tiles - shard_index) / shard_count) * 192 elements and a gather moves 1/shard_count of the frame. */
#define RTW_FLAG_COMPACT_TILES 2
/* RTW_FLAG_SCAN_VALU: run the plain scan entirely on the vector ALUs (the contract discriminant for every
 * sphere and every ray, 11 instructions each).  Default (0): pass 1 of the plain scan is a conservative filter
 * on the matrix pipe (v_mfma_f32_32x32x16_f16 over f16-split features), ~2.3x faster; the
 * exact contract test still decides every hit, so the image is the same bit for bit.  For A/B measurements
 * and as the reference the filter is tested against; also what the library uses by itself for scenes whose
 * extent the f16 split cannot cover (|coordinates| or radii beyond 2^40 or all below 2^-40). */
#define RTW_FLAG_SCAN_VALU 4
/* RTW_FLAG_RAY_POOL (Float32 plain scans on the matrix pipe; ignored otherwise): trace with the ray-pool kernel (rtw_pool.hpp) -- the
 * rays of a workgroup are parked in LDS between the stages scan / shade / path end and every stage runs on full waves of one
 * kind, instead of every lane keeping its own ray from the camera to the sky (rtw_kernels.hpp, the default).  Scheduling only:
 * the image is identical bit for bit.  Measured 14 % SLOWER than the default on MI355X (DESIGN.md section 6.4 says why); kept as
 * an independent cross-check of the default kernel and as the starting point for hardware with more LDS per CU. */
#define RTW_FLAG_RAY_POOL 8
/* RTW_FLAG_RCCL_REDUCE (rtw_render_f32/_f64 with a device list): every device renders its tiles into a zero-padded full frame and
 * ONE ncclReduce(sum, root = the first device of the list) over xGMI assembles the image (BASELINE configs[3]: "tile-sharded + RCCL
 * framebuffer reduce"; x + 0 == x, so the sum is the image bit for bit).  librccl is loaded on demand (dlopen; RTW_RCCL_LIB overrides
 * the path), one communicator per device list is kept until rtw_shutdown().  The devices of the list must be distinct.  Default (0):
 * compact shards gathered with peer copies (1/N of a frame per device instead of a whole one). */
#define RTW_FLAG_RCCL_REDUCE 16
/* The deciding arithmetic of the ray-sphere test, src/hit.jl:16-18.  In Float32 the choice is visible: on
 * scene_random_spheres the contract form traces 4 % fewer ray segments per sample than the reference's own order and its image is
 * brighter by 0.003 in the mean (fewer tmin re-hits of the r = 1000 ground sphere); Float64 images agree to the last few ulps.
 *   default (neither bit)            `oc . r.dir` and `oc . oc` as StaticArrays' dot evaluates them -- (x1 y1 + x2 y2) + x3 y3, no FMA:
 *                                    a callee, which @fastmath does not rewrite --, c = oc.oc - r^2, disc = half_b^2 - c, one rounding each
 *   RTW_FLAG_NUMERICS_REFERENCE_FMA2 the un-fused dots with BOTH squares contracted, disc = fma(half_b, half_b, -c) and c = fma(-r, r, oc.oc): what LLVM emits for an FMA target when BOTH squares of lines 17-18 carry
 *                                    fast-math flags (tools/llvm_fastmath_check/: with the flag-less llvm.powi of Julia's pow_fast neither site is fused)
 *   RTW_FLAG_NUMERICS_CONTRACT       ABI 2's arithmetic: half_b, r^2 - |oc|^2 and disc as three FMA chains
 * The bits exclude each other.  tools/julia_kat.jl + tools/check_julia_kat.py decide between them on a Julia box. */
#define RTW_FLAG_NUMERICS_CONTRACT 32
/* (64 was RTW_FLAG_NUMERICS_REFERENCE_FMA in ABI 3 -- only the last step contracted: removed in ABI 4, neither LLVM experiment of
 *  tools/llvm_fastmath_check/ emits it; the bit is rejected as unknown) */
#define RTW_FLAG_NUMERICS_REFERENCE_FMA2 128
/* Measurement / test switches of the ENVIRONMENT (RTW_SCAN, RTW_POOL, RTW_JOB_PIXELS, RTW_ROWS_SHIFT, RTW_NO_HUGE, RTW_PLAIN_ORDER,
 * RTW_DEBUG_REMOTE_SHARDS, RTW_DEBUG_NO_PEER, RTW_PHASE_PROFILE, RTW_DRAIN_PROFILE, RTW_DEBUG) are honoured only when the master switch
 * RTW_ENABLE_TEST_AIDS=1 is set too (read once per process).  Without it a stray variable changes nothing: a render's kernel choice, launch
 * geometry and gather path depend on rtw_params alone. */
/* rtw_stats_t.gather_path (bits): how the shards of the last multi-device render reached the first device */
#define RTW_GATHER_PEER 1         /* hipMemcpyPeerAsync with peer access enabled in both directions (xGMI)      */
#define RTW_GATHER_HOST_STAGED 2  /* no peer access on this platform: D2H into pinned memory, H2D on the root   */
#define RTW_GATHER_RCCL 4         /* ncclReduce (RTW_FLAG_RCCL_REDUCE)                                           */
#define RTW_GATHER_SAME_DEVICE 8  /* a shard on the root's own device rendered straight into the gather buffer   */

/* Positional arguments of render() plus the keyword extras of the shim. */
typedef struct {
    int32_t width;        /* image_width  (src/render.jl:8)                                   */
    int32_t height;       /* image_width div 16//9 (src/render.jl:11-12); computed by caller  */
    int32_t spp;          /* n_samples    (src/render.jl:9)                                   */
    int32_t max_depth;    /* ray_color depth; reference default 16 (src/ray_color.jl:14)      */
    uint64_t seed;        /* render seed; the stream of (pixel, chunk) derives from it        */
    int32_t n_chunks;     /* sample chunks per pixel, each with its own RNG stream;
                             0 = default rule min(spp, 256) (ABI <= 3: min(spp, clamp(spp / 4, 16, 256)): the default images of
                             renders with 17 .. 1023 spp changed with ABI 4; 1000 spp: 250 chunks either way).  Part of the image definition
                             (the sample radiances themselves are added exactly, in any order). */
    int32_t shard_index;  /* this call renders the 8x8 pixel tiles t with                      */
    int32_t shard_count;  /*   t mod shard_count == shard_index; other pixels are written 0    */
    int32_t device;       /* HIP device ordinal; -1 = current device                          */
    int32_t gamma;        /* 1 = sqrt per channel (rgb_gamma2, src/vec.jl:22); 0 = linear mean */
    int32_t flags;        /* 0, or RTW_FLAG_* (opt-in modes; the image is identical in every mode)    */
    int32_t n_devices;    /* rtw_render_f32/_f64 only (Julia keyword `devices`): 0 (or 1 with device_ids null) = the one
                             device named by `device`; N >= 1 = the N ordinals in device_ids; -1 = every visible
                             device.  The 8x8 tiles are dealt round-robin to the devices (a stream each); the
                             shards are gathered in HBM of the first device of the list -- peer copies with peer
                             access enabled per device pair (xGMI), a host-staged copy where the platform refuses
                             it; RTW_FLAG_RCCL_REDUCE: one ncclReduce instead -- and the frame is copied to `out`
                             once.  The image is identical for every device list; rtw_stats_t.gather_path says
                             which path ran. */
    int32_t job_pixels;   /* 0 = automatic.  1, 4, 8 or 16: pixels per work-queue job (1x1, 4x1, 8x1, 8x2: rows x columns).
                             Scheduling granularity only -- the image is identical for every value.      */
    const int32_t *device_ids; /* n_devices > 1: HIP ordinals; an ordinal may repeat (its shards then run
                             concurrently on that device)                                               */
} rtw_params;

/* Counters of the most recent render issued from the calling thread (summed over its devices;
 * times are the maximum over the devices). */
typedef struct {
    uint64_t samples;       /* pixel samples taken by this shard                              */
    uint64_t segments;      /* ray segments == closest-hit scans (src/hit.jl:38-50)           */
    uint64_t sphere_tests;  /* segments * n spheres (src/hit.jl:12-35 evaluations)            */
    double kernel_ms;       /* HIP-event time of the trace kernel (the only kernel of a render) */
    double total_ms;        /* same (kept from ABI 1, where a second kernel stored the image)  */
    int32_t n_chunks;       /* chunks per pixel actually used                                 */
    int32_t grid_blocks;    /* trace kernel launch geometry                                   */
    int32_t block_threads;
    int32_t gather_path;    /* multi-device renders: RTW_GATHER_* bits; 0 otherwise                  */
} rtw_stats_t;

int rtw_abi_version(void);
int rtw_device_count(int *count);
const char *rtw_last_error(void);

/* render(scene, cam, width, spp) for elem_type Float32 / Float64 -- replaces
 * /root/reference/src/render.jl:8-44.  `out` is a HOST buffer of height*width*3 elements in
 * the memory layout of the returned Matrix{RGB{T}}: pixel (i,j) (1-based row, column) at
 * ((j-1)*height + (i-1))*3.  Blocking.  Uploads the scene, renders, copies the image back.
 * The library keeps the uploaded scene (recognised by its bytes), a stream and the device image per
 * device between calls: from the second call of a scene on, a call costs its kernel + one D2H of the
 * image (0.5 ms at 1920x1080 Float32).  rtw_shutdown() releases them. */
int rtw_render_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cam, const rtw_params *p,
                   float *out);
int rtw_render_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cam, const rtw_params *p,
                   double *out);

/* Device-resident variant of the same call for callers that keep the image in HBM (bench.py,
 * multi-process sharding over RCCL).  `scene` is a handle from rtw_scene_upload_*; `d_out` is a
 * DEVICE pointer to height*width*3 elements; `hip_stream` is a hipStream_t passed as void*
 * (NULL = the null stream).  Asynchronous with respect to the host: work is enqueued on the
 * stream and nothing is waited for; rtw_stats() synchronises with it.  Re-entrant: any number of
 * renders may be in flight on any mix of streams, host threads and devices (each call owns its
 * counters; there is no shared device workspace). */
typedef struct rtw_scene_dev *rtw_scene_handle;
int rtw_scene_upload_f32(const rtw_scene_f32 *scene, int device, rtw_scene_handle *out);
int rtw_scene_upload_f64(const rtw_scene_f64 *scene, int device, rtw_scene_handle *out);
int rtw_scene_free(rtw_scene_handle scene);
int rtw_render_device_f32(rtw_scene_handle scene, const rtw_camera_f32 *cam, const rtw_params *p,
                          void *d_out, void *hip_stream);
int rtw_render_device_f64(rtw_scene_handle scene, const rtw_camera_f64 *cam, const rtw_params *p,
                          void *d_out, void *hip_stream);

/* Batched render: N views of ONE scene -- same size, spp, depth, flags -- in one kernel launch (turntables, animation frames,
 * multi-view datasets).  View v is bit-identical to rtw_render_* with cams[v] and seed seeds[v] (seeds == NULL: p->seed for every
 * view) in every mode.  `cams` is a HOST array of n_views cameras; `out` / `d_out` hold n_views consecutive frames of the layout above:
 * pixel (i, j) of view v at ((v*width + j-1)*height + i-1)*3 (Julia's Array{RGB{T},3} of size (height, width, n_views)).  The host
 * variant keeps the same per-device cache as rtw_render_f32 and does one D2H; the device variant is asynchronous like
 * rtw_render_device_*.  rtw_stats() afterwards reports the batch: samples = N*W*H*spp, the summed segments, one kernel time.
 * One device and whole frames only: shard_count != 1, RTW_FLAG_COMPACT_TILES, RTW_FLAG_RCCL_REDUCE, RTW_FLAG_RAY_POOL, n_devices > 1 or
 * device_ids -> -2; n_views < 1 -> -2; a null cams / out -> -1; a batch whose jobs the queues cannot number -> -5 (all decided before any
 * HIP call).  Additive to ABI 4: callers detect it by symbol lookup. */
int rtw_render_batch_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_views,
                         const uint64_t *seeds, const rtw_params *p, float *out);
int rtw_render_batch_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_views,
                         const uint64_t *seeds, const rtw_params *p, double *out);
int rtw_render_batch_device_f32(rtw_scene_handle scene, const rtw_camera_f32 *cams, int32_t n_views,
                                const uint64_t *seeds, const rtw_params *p, void *d_out, void *hip_stream);
int rtw_render_batch_device_f64(rtw_scene_handle scene, const rtw_camera_f64 *cams, int32_t n_views,
                                const uint64_t *seeds, const rtw_params *p, void *d_out, void *hip_stream);

/* Progressive render: a render added up pass by pass in an EXACT accumulator -- a picture that sharpens while it is watched, a render
 * that stops at a time budget, survives a restart (export / import) or has its samples split over streams, devices or processes.
 *
 * The contract: samples are grouped in chunks whose random streams depend on (seed, pixel, chunk) only, and every sample is added as a
 * signed 64.64 fixed-point integer, so ANY partition of a render's chunks into passes -- in any order, in any mix of RTW_FLAG_GROUP_CULL /
 * RTW_FLAG_SCAN_VALU / job_pixels, on one accumulator or merged from several -- resolves to the image of the single rtw_render_* call,
 * bit for bit.  Every prefix is itself a render: after the chunks [0, C) of a render (spp = S, chunk size s) the image equals rtw_render_*
 * with spp = min(S, C*s), n_chunks = C.
 *
 * The accumulator: width*height pixels x 8 uint64_t in device memory, pixel (i, j) (1-based row, column) at word ((j-1)*height + (i-1))*8:
 *     r_lo, r_hi, g_lo, g_hi, b_lo, b_hi, poison, 0          (word 7: the half difference of an ADAPTIVE accumulator, see below)
 * (lo, hi) = the channel's sum of radiances as a two's-complement 128-bit integer in units of 2^-64, each radiance truncated towards zero
 * at 2^-64; poison = the number of channel values that were not finite or beyond 2^31 (such a pixel resolves to NaN, as in rtw_render_*).
 *
 * rtw_render_accum_*: `p` describes the WHOLE render (spp, n_chunks with the default rule of rtw_params, seed, max_depth, numerics bits);
 * the call renders the chunks [chunk_begin, chunk_begin + chunk_count) of it -- in units of the effective chunks, rtw_stats_t.n_chunks of
 * the whole render = rtw_accum_info_t.n_chunks -- and adds them to `a`.  d_out != NULL: the running image (layout of rtw_render_device_*,
 * p->gamma) is written from the new sums, divided by the samples the accumulator holds INCLUDING this pass.  Asynchronous like
 * rtw_render_device_*; rtw_stats() afterwards reports this pass alone.  Operations on one accumulator are ordered by the library in the
 * order of the calls whatever their streams (each waits for the previous one on the device); the calls themselves must not run
 * concurrently on one accumulator.  Two streams that should overlap -> two accumulators -> rtw_accum_merge.
 *   The first pass BINDS the accumulator to its render: size, precision, seed, spp, chunk size, n_chunks, max_depth, numerics bits, the
 * camera's bytes and a 64-bit hash of the scene's arrays taken at upload.  The host keeps the chunk ranges already added.  A later pass,
 * or a merge, of another render -> -4; a range that overlaps what is there -> -2; both before any HIP call, the accumulator untouched.
 * RTW_FLAG_GROUP_CULL, RTW_FLAG_SCAN_VALU, job_pixels and gamma may differ from pass to pass.  rtw_accum_reset zeroes and unbinds.
 *   Whole frames on one device: shard_count != 1, RTW_FLAG_COMPACT_TILES, RTW_FLAG_RCCL_REDUCE, RTW_FLAG_RAY_POOL, n_devices > 1 or
 * device_ids -> -2; chunk_begin < 0, chunk_count < 1 or a range beyond the effective n_chunks -> -2; a null cam / p / accumulator /
 * scene -> -1 (these, in this order, before the handles are looked at); a scene of the other precision, an accumulator of another size
 * or device than the call -> -4.  All decided before any HIP call.
 *   rtw_accum_resolve_*: accumulator -> image (sum / samples held, sqrt if gamma, rounded to T) into DEVICE memory, asynchronous;
 * _host_: into HOST memory, blocking.  An accumulator without samples -> -2; the other precision than its render's -> -4.
 *   rtw_accum_merge: dst += src (same size and device, else -4; disjoint chunk ranges of the same render, else -4 / -2, dst untouched;
 * an unbound dst takes src's binding; an unbound src is a no-op).  Asynchronous on `hip_stream`, ordered behind both accumulators' work.
 *   rtw_accum_ranges: the chunk ranges held, sorted, disjoint and coalesced: *count receives their number, at most `capacity` pairs
 * (begin, end), end exclusive, are written to begin_end.
 *   rtw_accum_read_pixels: blocking copy of the words (layout above) to the host, behind everything enqueued on the accumulator.
 *   rtw_accum_export: blocking; writes a self-describing, versioned blob -- the bound render, the chunk ranges, the words -- of *size
 * bytes (buf == NULL: only reports *size; capacity < *size -> -2).  rtw_accum_import recreates the accumulator from it on any device:
 * the checkpoint, and the way partial sums travel between devices or processes (there is no cross-device merge in the library).  A
 * truncated blob, one of another version or a corrupt one -> -2, before any HIP call.  Blobs are little-endian like the device.
 *   Accumulators own their device memory: rtw_shutdown() does NOT invalidate them.  Additive to ABI 4: detected by symbol lookup. */
typedef struct rtw_accum *rtw_accum_handle;
typedef struct {
    int32_t width, height, device;
    int32_t bound;          /* 0: no pass yet (the fields below are 0)                        */
    int32_t precision;      /* 32 or 64                                                       */
    int32_t spp, chunk_spp; /* of the whole render; chunk_spp = samples per chunk             */
    int32_t n_chunks;       /* effective chunks of the whole render                           */
    int32_t max_depth;
    int32_t numerics_flags; /* the RTW_FLAG_NUMERICS_* bits of the render                     */
    int32_t chunks_done;    /* chunks held                                                    */
    int32_t samples_done;   /* samples per pixel held: the divisor of resolve                 */
    int32_t complete;       /* chunks_done == n_chunks                                        */
    uint64_t seed;
} rtw_accum_info_t;
int rtw_accum_create(int device, int32_t width, int32_t height, rtw_accum_handle *out);   /* zeroed */
int rtw_accum_reset(rtw_accum_handle a, void *hip_stream);
int rtw_accum_free(rtw_accum_handle a);
int rtw_render_accum_f32(rtw_scene_handle scene, const rtw_camera_f32 *cam, const rtw_params *p,
                         int32_t chunk_begin, int32_t chunk_count, rtw_accum_handle a, void *d_out, void *hip_stream);
int rtw_render_accum_f64(rtw_scene_handle scene, const rtw_camera_f64 *cam, const rtw_params *p,
                         int32_t chunk_begin, int32_t chunk_count, rtw_accum_handle a, void *d_out, void *hip_stream);
int rtw_accum_resolve_f32(rtw_accum_handle a, int32_t gamma, void *d_out, void *hip_stream);
int rtw_accum_resolve_f64(rtw_accum_handle a, int32_t gamma, void *d_out, void *hip_stream);
int rtw_accum_resolve_host_f32(rtw_accum_handle a, int32_t gamma, float *out);
int rtw_accum_resolve_host_f64(rtw_accum_handle a, int32_t gamma, double *out);
int rtw_accum_merge(rtw_accum_handle dst, rtw_accum_handle src, void *hip_stream);
int rtw_accum_info(rtw_accum_handle a, rtw_accum_info_t *out);
int rtw_accum_ranges(rtw_accum_handle a, int32_t capacity, int32_t *count, int32_t *begin_end);
int rtw_accum_read_pixels(rtw_accum_handle a, uint64_t *host_words);
int rtw_accum_export(rtw_accum_handle a, void *buf, uint64_t capacity, uint64_t *size);
int rtw_accum_import(int device, const void *buf, uint64_t size, rtw_accum_handle *out);

/* Adaptive sampling: a progressive render that stops each 8x8 tile as soon as an EXACT noise estimate says it is good enough.
 *
 * The definition.  An adaptive render is a progressive render (spp = S, effective n_chunks = N, chunk size s) in which every 8x8 tile t
 * ends up holding a prefix [0, C_t) of the chunks.  Tiles are numbered column-major like the image, t = tj*tiles_i + ti (tiles_i =
 * ceil(height / 8) tiles down a column); ragged tiles at the frame's edges count their valid pixels only.
 *   Checkpoints: the chunk counts c = min_chunks, min_chunks + check_chunks, ... below N.  min_chunks and check_chunks are even and >= 2
 * (the two halves below then hold equally many FULL chunks at every checkpoint); 0 = the default, the smallest even number >=
 * max(16, N/8) (passes of fewer than 16 chunks are in the launcher's bad regime).
 *   Noise statistic: for every sample and channel q = min(fx >> 40, 2^30 - 1), fx = the channel's 64.64 fixed-point radiance exactly as
 * it is added to the sums (so q is in units of 2^-24 and capped at 64); q = 0 for a negative or a poisoning value.  The pixel's HALF
 * DIFFERENCE H_p is the signed 64-bit sum of +q over the samples of even global chunks and -q over the samples of odd global chunks
 * (|H_p| < 2^63 for any int32 sample count).  It lives in word 7 of the pixel's record -- 0 in every other accumulator -- and, being an
 * integer sum, does not depend on order, scan mode, job size or pass structure.
 *   Stopping rule: at checkpoint c a tile with C_t == c holds n = c*s samples per pixel and has npix valid pixels; it is CONVERGED iff
 *         D <= tol * max(Y, floor * n * npix)
 *     D = sum_p (double)|H_p| * 2^-24,   Y = sum_p max(y_p, 0),   y_p = (double(R) + double(G)) + double(B)
 * (double(.) = the channel's 128-bit sum rounded once to binary64, as resolve does), both sums over the tile's valid, unpoisoned pixels in
 * the tile-local order (i mod 8) + 8 (j mod 8) -- a poisoned pixel adds 0 to both.  Everything in binary64, every operation rounded once,
 * no FMA, the sums sequential in that order; the right-hand side is ((floor * (double)n) * (double)npix), then max, then * tol.
 *   C_t = the first checkpoint at which tile t is converged, else N.
 *   (Approximately -- not part of the contract: D / Y = 1/2 sum|mean_even - mean_odd| / sum mean, so for a tile of pixels of similar
 * noise `tolerance` is roughly 0.8 x the tile's relative standard error; dark_floor keeps near-black tiles from never stopping: it is
 * the radiance per sample and pixel, summed over the channels, below which the tile is judged as if it were that bright.)
 *   Consequences (tests/test_gpu_adaptive.py): tile t of the adaptive image equals, bit for bit, tile t of rtw_render_* with spp =
 * min(S, C_t*s), n_chunks = C_t; image and C_t are identical in every mix of RTW_FLAG_GROUP_CULL, RTW_FLAG_SCAN_VALU and job_pixels;
 * REFINEMENT is exact: continuing an adaptive accumulator with a tolerance <= the previous one, all else equal, gives the words and C_t
 * of a fresh run at the new tolerance (a tile that passes the tighter test passed the looser one no later).
 *
 * rtw_render_adaptive_*: `p` describes the whole render as for rtw_render_accum_*.  The call runs the whole loop -- a pass over the chunks
 * [0, min_chunks) of all tiles, a check, a pass over the tiles still active, ... until no tile is active or the chunks run out -- and is
 * BLOCKING: it returns when the image is complete (each round reads the number of active tiles back: one 4-byte copy).  d_out != NULL
 * (device memory, layout of rtw_render_device_*, p->gamma) receives the final image, each pixel divided by the samples its tile holds.
 * rtw_stats() afterwards reports the sums over all rounds (kernel_ms: the sum of the passes' kernels).  The accumulator must be unbound,
 * or an adaptive accumulator of the same render with the same dark_floor, min_chunks and check_chunks and a `tolerance` <= its last one:
 * that is refinement.  rtw_accum_resolve_*, rtw_accum_read_pixels, rtw_accum_info and rtw_accum_ranges work on an adaptive accumulator:
 * resolve divides per tile; chunks_done, samples_done and the range report the LEAST sampled tile; complete = no tile is active under
 * the last tolerance.  rtw_accum_reset clears the adaptive state with everything else.
 *   Refusals, all decided before any HIP call, the accumulator untouched: a null scene / cam / p / adaptive / accumulator -> -1;
 * tolerance not finite or <= 0, dark_floor not finite or < 0, min_chunks or check_chunks odd or < 0 -> -2; the whole-frame, one-device
 * restrictions of rtw_render_accum_* -> -2; an accumulator bound by plain passes, by another render or other dark_floor / min_chunks /
 * check_chunks, or a looser tolerance than its last -> -4.  rtw_render_accum_*, rtw_accum_merge (either side) and rtw_accum_export on
 * an adaptive accumulator -> -2: per-tile chunk ranges in passes, merges and blobs are out of scope.
 *   rtw_accum_adaptive_info: the state of an adaptive accumulator (-2 for any other).  rtw_accum_tile_chunks: *count receives the number
 * of tiles, at most `capacity` values C_t are written to `chunks` in tile order (an accumulator that is not adaptive reports its
 * chunks_done for every tile when its ranges are one prefix [0, C), else -2).  Additive to ABI 4: detected by symbol lookup. */
typedef struct {
    double tolerance;       /* > 0; smaller = more samples                                                      */
    double dark_floor;      /* >= 0; radiance per sample and pixel (R + G + B) below which a tile counts as that bright */
    int32_t min_chunks;     /* first checkpoint: even, 0 = default                                                */
    int32_t check_chunks;   /* distance of the checkpoints: even, 0 = default                                     */
    int32_t reserved[2];    /* 0                                                                                  */
} rtw_adaptive_t;
typedef struct {
    int32_t n_tiles;          /* tiles of the frame                                                               */
    int32_t tiles_converged;  /* tiles that stopped by the rule (C_t < N)                                         */
    int32_t tiles_at_cap;     /* tiles that hold all N chunks                                                     */
    int32_t rounds;           /* passes of the last call                                                          */
    int32_t min_chunks_held;  /* min C_t                                                                          */
    int32_t max_chunks_held;  /* max C_t                                                                          */
    uint64_t samples;         /* sum over the tiles of valid pixels x min(S, C_t*s): every sample in the accumulator */
    double tolerance;         /* of the last call                                                                 */
} rtw_adaptive_info_t;
int rtw_render_adaptive_f32(rtw_scene_handle scene, const rtw_camera_f32 *cam, const rtw_params *p, const rtw_adaptive_t *adaptive,
                            rtw_accum_handle a, void *d_out, void *hip_stream);
int rtw_render_adaptive_f64(rtw_scene_handle scene, const rtw_camera_f64 *cam, const rtw_params *p, const rtw_adaptive_t *adaptive,
                            rtw_accum_handle a, void *d_out, void *hip_stream);
int rtw_accum_adaptive_info(rtw_accum_handle a, rtw_adaptive_info_t *out);
int rtw_accum_tile_chunks(rtw_accum_handle a, int32_t capacity, int32_t *count, int32_t *chunks);

/* Batched progressive and adaptive renders: N views of ONE scene -- same size, spp, chunks, depth, flags -- each with its own accumulator,
 * every pass ONE kernel launch for all of them (an adaptive turntable or animation: `rounds` launches and host waits instead of
 * N x rounds, and late passes N times as full).
 *
 * The contract: accumulator v after a batched call is indistinguishable from the same accumulator after the single-view call with cams[v],
 * seed seeds[v] (seeds == NULL: p->seed for every view) and the same p / adaptive -- the same words (word 7 included), the same C_t, the same
 * binding, the same answer from every query, all on the bits.  Each accumulator is afterwards an ordinary progressive or adaptive
 * accumulator: it can be continued alone or in another batch, in any mix.
 *   `cams`, `seeds` and `accums` are HOST arrays of n_views entries.  d_out != NULL receives n_views frames in the layout of
 * rtw_render_batch_device_*.  The calls are ordered on EVERY accumulator of the array (they wait for all n_views accumulators' previous
 * operations and are waited for by all their next ones).  rtw_stats() afterwards reports the sums over the views (and, adaptive, over
 * the rounds).
 *   rtw_render_accum_batch_*: the chunks [chunk_begin, chunk_begin + chunk_count) of every view's render in ONE launch, added to
 * accums[v]; asynchronous like rtw_render_accum_*.  Every accumulator is validated on its own exactly as rtw_render_accum_* validates it:
 * unbound or bound to its own view's render, the range not overlapping what IT holds; the accumulators may hold different ranges before
 * the call.  Frame v of d_out is divided by the samples accums[v] holds including this pass.  The first pass binds accums[v] to
 * (cams[v], seeds[v], p).  rtw_accum_merge / export / import / resolve / info / ranges work on each accumulator as ever.
 *   rtw_render_adaptive_batch_*: blocking like rtw_render_adaptive_*; ONE loop for all views: a pass over [0, min_chunks) of all tiles of
 * all views; at each checkpoint ONE check over the n_views x n_tiles tiles, ONE sorted list of the active batch-global tiles
 * (v * n_tiles + t), ONE 4-byte read-back and ONE pass over that list; until no view has an active tile or the chunks run out.  The
 * accumulators are all unbound, or all adaptive accumulators of their own views' renders with the call's dark_floor / min_chunks /
 * check_chunks and a last tolerance >= the call's (refinement).  rtw_accum_adaptive_info(accums[v]).rounds is what the single call
 * reports: the passes of this call that held at least one tile of view v.
 *   Refusals, all decided before any HIP call with NO accumulator of the array touched: a null scene / cams / p / adaptive / accums or a
 * null entry of accums -> -1; n_views < 1, the whole-frame one-device restrictions of rtw_render_batch_* and rtw_render_accum_*, a bad
 * chunk range, bad adaptive parameters, one accumulator twice in the array, a range overlapping what some accumulator holds,
 * rtw_render_accum_batch_* on an adaptive accumulator -> -2; a batch whose jobs the queues cannot number (rtw_render_batch_*) -> -5; an
 * accumulator of another size, device or precision, one bound to another render than its view's, a mix of unbound and bound accumulators
 * in the adaptive call, a looser tolerance than some accumulator's last -> -4.  Additive to ABI 4: detected by symbol lookup. */
int rtw_render_accum_batch_f32(rtw_scene_handle scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds,
                               const rtw_params *p, int32_t chunk_begin, int32_t chunk_count,
                               const rtw_accum_handle *accums, void *d_out, void *hip_stream);
int rtw_render_accum_batch_f64(rtw_scene_handle scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds,
                               const rtw_params *p, int32_t chunk_begin, int32_t chunk_count,
                               const rtw_accum_handle *accums, void *d_out, void *hip_stream);
int rtw_render_adaptive_batch_f32(rtw_scene_handle scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds,
                                  const rtw_params *p, const rtw_adaptive_t *adaptive,
                                  const rtw_accum_handle *accums, void *d_out, void *hip_stream);
int rtw_render_adaptive_batch_f64(rtw_scene_handle scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds,
                                  const rtw_params *p, const rtw_adaptive_t *adaptive,
                                  const rtw_accum_handle *accums, void *d_out, void *hip_stream);

/* First-hit feature buffers: per pixel the surface colour, normal and depth of what the camera sees first, and how much of the pixel is
 * covered -- the guides that denoisers, edge-aware upsamplers and compositing steps want next to a low-sample-count image (a progressive
 * prefix, an adaptive render).  Defined on the render's own primary rays, exact like the image itself.
 *
 * The definition.  A render `p` (width W, height H, spp = S, seed, numerics bits, camera) has N effective chunks of s = ceil(S / n_chunks)
 * samples under the default rule of rtw_params.n_chunks (N = rtw_stats_t.n_chunks of the render).  Chunk c of pixel (i, j) (1-based row,
 * column) starts with the random stream of (seed, pix, c), pix = (j-1)*H + (i-1), and its first sample has the global index c*s.  The
 * FEATURE SAMPLE of (pixel, chunk c) is the primary ray of that first sample, built exactly as the render builds it: the jitter is drawn
 * iff c*s != 0 -- du = rand / T(Float32(W)), then dv = rand / T(Float32(H)) --, then get_ray(cam, T(j/W) + du, T((H-i)/H) + dv) with its
 * lens-disk rejection drawn from the same stream (src/render.jl:26-37, src/camera.jl:43-48), then hit(world, ray, T(1e-4), typemax(T)) in
 * the render's numerics mode, ties resolved as the render's scans resolve them (the later sphere of the caller's list).  With s == 1 these
 * are all the primary rays of the image, otherwise every s-th.  Each feature sample contributes 8 binary64 values:
 *     slot 0-2  albedo    hit: the attenuation of scatter() (src/material.jl: the albedo of a Lambertian / Metal, (1, 1, 1) for a Dielectric), widened
 *                         miss: skycolor(ray) as the render adds it (src/ray_color.jl:1-6, binary64)
 *     slot 3-5  normal    hit: HitRecord.n, the face-forwarded normal (src/hit.jl:6-10; a negative radius flips the outward normal), widened; miss: 0
 *     slot 6    depth     hit: HitRecord.t, widened; miss: 0
 *     slot 7    coverage  hit: 1; miss: 0
 * The values of the chunks [chunk_begin, chunk_begin + chunk_count) are summed per slot as signed 64.64 fixed-point integers, exactly as the
 * render sums radiances (each value truncated towards zero at 2^-64; a value that is not finite or beyond 2^31 poisons the pixel); each sum
 * is rounded once to binary64, divided by (double)chunk_count and the quotient rounded to T.  No gamma.  Normals are NOT renormalised and
 * depth is averaged over ALL samples of the range, hits or not: the caller divides both by coverage.  A poisoned pixel is NaN in all 8 slots.
 * Layout: pixel-interleaved, pixel (i, j) at ((j-1)*H + (i-1)) * RTW_FEATURE_CHANNELS -- Julia's Array{T,3} of size (8, H, W).
 *   The result depends on p (size, spp, n_chunks, seed, numerics bits), the camera, the scene and the chunk range only: RTW_FLAG_GROUP_CULL,
 * RTW_FLAG_SCAN_VALU and every legal job_pixels are accepted and give identical words; max_depth and gamma are ignored (but validated).
 *
 * rtw_render_features_device_*: `d_out` is a DEVICE pointer, 16-byte aligned, to height*width*8 elements; asynchronous like
 * rtw_render_device_*.  rtw_render_features_*: `out` is a HOST buffer of that size; blocking; the per-device scene, stream and buffer cache
 * of rtw_render_f32.  rtw_stats() afterwards reports this call: samples = segments = W*H*chunk_count (one scan per pixel and chunk),
 * sphere_tests = segments * n, n_chunks = N, the kernel's HIP-event time.
 *   Refusals, all decided before any HIP call and before a handle is looked at: a null scene / cam / p / output -> -1; the usual validation of
 * rtw_params -- sizes, unknown flags, both numerics bits, job_pixels -> -2; chunk_begin < 0, chunk_count < 1 or a range beyond N -> -2;
 * shard_count != 1, RTW_FLAG_COMPACT_TILES, RTW_FLAG_RCCL_REDUCE, RTW_FLAG_RAY_POOL, n_devices > 1 or device_ids -> -2; a d_out that is not
 * 16-byte aligned -> -2; a frame of 2^31 tiles or more -> -5.  Then: a scene handle of the other precision, or on another device than
 * p->device names -> -4.  Feature sums in accumulators and device lists are out of scope; N views in one launch:
 * rtw_render_features_batch_* below; the
 * per-tile chunk prefixes of an adaptive accumulator: rtw_accum_features_* below.  Additive to ABI 4: detected by symbol lookup. */
#define RTW_FEATURE_CHANNELS 8
int rtw_render_features_device_f32(rtw_scene_handle scene, const rtw_camera_f32 *cam, const rtw_params *p,
                                   int32_t chunk_begin, int32_t chunk_count, void *d_out, void *hip_stream);
int rtw_render_features_device_f64(rtw_scene_handle scene, const rtw_camera_f64 *cam, const rtw_params *p,
                                   int32_t chunk_begin, int32_t chunk_count, void *d_out, void *hip_stream);
int rtw_render_features_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cam, const rtw_params *p,
                            int32_t chunk_begin, int32_t chunk_count, float *out);
int rtw_render_features_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cam, const rtw_params *p,
                            int32_t chunk_begin, int32_t chunk_count, double *out);

/* Feature-guided denoiser: an edge-avoiding a-trous filter of a low-sample-count image, guided by the first-hit feature buffers above.
 *
 * The definition.  Everything is computed in the element type T (binary32 or binary64); every operation is rounded once, no FMA, no
 * reassociation; quotients and the final sqrt are the correctly rounded IEEE ones.  Inputs: `image`, H*W*3 in the layout of the render
 * entry points (normally a gamma = 0 image), and `features`, H*W*8 in the layout of the feature entry points; pixel (i, j) (0-based row,
 * column) at j*H + i.  Call the pixel's colour c[0..2] and its feature slots f[0..7].
 *   Prepare, per pixel p.  valid(p): all 3 + 8 inputs are finite.  cov = f[7]; has(p) = valid and cov > 0.  If has: n = f[3..5] / cov
 * (three quotients) and z = f[6] / cov, otherwise n = 0 and z = 0.  With RTW_DENOISE_DEMODULATE: a[k] = max(f[k], T(2^-6)) and
 * e[k] = c[k] / a[k], k = 0..2; otherwise a = 1 and e = c.
 *   Level k = 0 .. levels-1, step s = 2^k.  The host computes in binary64 sc = sigma_color * 2^-k, inv_sc = T(1.0 / (sc*sc)) and
 * inv_sz = T(1.0 / (sigma_depth*sigma_depth)).  For every valid p: sum_w = +0, sum_e = (+0, +0, +0); the taps are visited with dj = -2..2
 * as the outer and di = -2..2 as the inner loop; the tap pixel is q = p + s*(di, dj); h = K[|di|] * K[|dj|] with K = (3/8, 1/4, 1/16)
 * (exact products).  The centre tap (di = dj = 0) has w = h = 9/64 and e_q = e_p.  A tap outside the frame, or whose q is not valid, is
 * skipped.  Any other tap:
 *       d = e_p - e_q;  dc = (d0*d0 + d1*d1) + d2*d2;  w_c = 1 / (1 + dc*inv_sc)
 *       t_v = 1 - |cov_p - cov_q|;  w_v = t_v > 0 ? t_v : +0
 *       w = (h*w_c)*w_v
 *       if has(p) and has(q):
 *           dot = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z;  t = dot > 0 ? dot : +0, then t = t*t repeated m = normal_power_log2 times
 *           zs = z_p + z_q;  r = (z_p - z_q) / (zs > 0 ? zs : 1);  w_z = 1 / (1 + (r*r)*inv_sz)
 *           w = (w*t)*w_z
 * Every visited tap accumulates sum_w = sum_w + w and sum_e[k] = sum_e[k] + w*e_q[k].  After the 25 taps e'_p[k] = sum_e[k] / sum_w
 * (sum_w >= 9/64).  All pixels of a level read the previous level's e; the guides n, z, cov and a never change.
 *   End.  out[k] = e[k] * a[k] with RTW_DENOISE_DEMODULATE, else e[k]; then sqrt if gamma = 1.  A pixel that is not valid is a quiet NaN
 * in all three channels, and it is never a neighbour.
 *   The weights are rational, not exponential, so that a CPU restatement agrees on the bits (tests/denoise_ref.py); the depth difference is
 * relative (the scenes have a ground sphere of radius 1000); the coverage term needs no parameter.
 *
 * The device form is asynchronous on `hip_stream` (a hipStream_t as void*; NULL = the null stream) of the device d->device (-1: the current
 * one).  The caller owns `d_work`: as many bytes as the work-bytes call below returns for the frame (a multiple of 16, monotone in the size;
 * < 0: an error code), 16-byte aligned; there is no shared device workspace, so any number of calls may be in flight with a workspace each.
 * `d_features` is 16-byte aligned, `d_image` and `d_out` are aligned to T; `d_out` may not alias an input or the workspace.  The host form
 * is blocking and uses the per-device stream and buffer cache of rtw_render_f32.  Neither changes what rtw_stats() reports: time them with
 * stream events.
 *   The render-and-denoise call renders `p` with gamma = 0, runs the feature pass over all N effective chunks of that render and the
 * denoiser with d->gamma replaced by p->gamma (and d->device by p->device), all on the cached context's stream, and copies the result to
 * `out` once.  rtw_stats() afterwards reports the render's record.
 *   Refusals, all decided before any HIP call: a null argument -> -1; levels outside 1..8, normal_power_log2 outside 0..7, unknown flag
 * bits, gamma other than 0 or 1, reserved != 0, device < -1, a sigma that is not finite and positive, width or height < 1, misaligned or
 * aliasing pointers, elem_bytes other than 4 or 8 -> -2; a frame of 2^31 8x8 tiles or more -> -5; the render-and-denoise call additionally
 * refuses everything a feature render of `p` refuses.  Compact or sharded frames and device lists are out of scope (DESIGN.md
 * section 9); history reuse across the views of a camera path: the rtw_temporal_* block further down; N frames in each launch: rtw_filter_batch_* below; noise-guided weights and accumulators as the input: the block behind these declarations.
 * Additive to ABI 4: detected by symbol lookup. */
#define RTW_DENOISE_DEMODULATE 1   /* filter image / albedo, multiply back at the end */
typedef struct {
    int32_t levels;             /* 1..8 a-trous passes; pass k has step 2^k */
    int32_t normal_power_log2;  /* 0..7: m, normal weight = max(0, n.n')^(2^m) */
    int32_t flags;              /* RTW_DENOISE_* */
    int32_t gamma;              /* 1 = sqrt per channel at the end, 0 = linear */
    int32_t device;             /* -1 = current */
    int32_t reserved;           /* 0 */
    double  sigma_color;        /* > 0, finite */
    double  sigma_depth;        /* > 0, finite */
} rtw_denoise_t;                /* 40 bytes */
int64_t rtw_denoise_work_bytes(int32_t width, int32_t height, int32_t elem_bytes);
int rtw_denoise_device_f32(const rtw_denoise_t *d, int32_t width, int32_t height, const void *d_image, const void *d_features,
                           void *d_out, void *d_work, void *hip_stream);
int rtw_denoise_device_f64(const rtw_denoise_t *d, int32_t width, int32_t height, const void *d_image, const void *d_features,
                           void *d_out, void *d_work, void *hip_stream);
int rtw_denoise_f32(const rtw_denoise_t *d, int32_t width, int32_t height, const float *image, const float *features, float *out);
int rtw_denoise_f64(const rtw_denoise_t *d, int32_t width, int32_t height, const double *image, const double *features, double *out);
int rtw_render_denoised_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cam, const rtw_params *p, const rtw_denoise_t *d, float *out);
int rtw_render_denoised_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cam, const rtw_params *p, const rtw_denoise_t *d, double *out);

/* Accumulators as the input of the filter above: the feature buffers of exactly the samples a progressive or adaptive accumulator holds,
 * a per-pixel noise map from the half differences of an adaptive accumulator, a form of the filter whose colour weight is scaled by that
 * map, and one call that strings them together.  Everything here only READS the accumulator's words and C_t; every call waits for the
 * accumulator's event on its stream and records it afterwards, like a resolve, so a later pass cannot overwrite them under a running kernel.
 *
 * rtw_accum_features_*: asynchronous like the device form of the feature pass above; `d_out` is a DEVICE pointer, 16-byte aligned, to
 * height*width*8 elements in the layout of the feature entry points.  `scene`, `cam` and `p` are the accumulator's render.
 *   Adaptive accumulator: tile t = tj*tiles_i + ti (the numbering of the adaptive render) receives the feature sums of the chunks
 * [0, C_t), every sum rounded once to binary64, divided by (double)C_t and rounded to T: the definition above with the tile's own range.
 * The kernel reads C_t from the accumulator's device array; its counters add valid pixels x C_t per tile (rtw_stats: samples = segments =
 * the sum over the tiles).  Consequence (tests/test_gpu_accum_denoise.py): the tiles with C_t == c equal, bit for bit, those tiles of
 * the device form of the feature pass above over [0, c).
 *   Uniform accumulator: it must hold exactly ONE chunk interval [b, b + C); the call is the feature pass above over it.
 *   Refusals, all before any HIP call: a null scene / cam / p / accumulator / d_out -> -1; everything the device form of the feature pass
 * refuses for `p` -> its code; a scene of the other precision, an accumulator of another size or device -> -4; an accumulator that holds
 * nothing -> -2; a scene, camera or parameter set that is not the accumulator's binding (the comparison a pass makes: size, precision,
 * seed, spp, chunk size, n_chunks, max_depth, numerics bits, the camera's bytes, the scene's hash) -> -4; RTW_FLAG_GROUP_CULL, RTW_FLAG_SCAN_VALU,
 * job_pixels and gamma may differ from the binding's (they do not change the words); a uniform accumulator that holds several intervals
 * -> -2; an adaptive accumulator whose last adaptive call did not finish -> -2.
 *
 * rtw_accum_noise_*: asynchronous; `d_out` is a DEVICE pointer to height*width elements of T, pixel (i, j) (0-based row, column) at
 * j*height + i.  Adaptive accumulators only (a uniform accumulator's word 7 is 0 by contract: -2; the other precision than its render's:
 * -4; a last adaptive call that did not finish: -2; nulls: -1; a misaligned d_out: -2).
 *   The definition, in binary64, one rounding per operation, no FMA.  For a pixel p in tile t whose poison word is 0, with the
 * accumulator's bound dark_floor, spp = S and chunk size s:
 *       n = min(S, C_t*s);   D = (double)|H_p| * 2^-24  (the magnitude as an unsigned value: INT64_MIN is 2^63);
 *       y = (double(R) + double(G)) + double(B)  as the stopping rule computes it;   M = max(max(y, 0), dark_floor * (double)n);
 *       rho_p = M > 0 ? D / M : 0.
 * The map is the 3 x 3 binomial mean of rho:  num = +0, den = +0; for dj = -1..1 (outer), di = -1..1 (inner), q = p + (di, dj) inside the
 * frame and not poisoned, b = (2 - |di|) * (2 - |dj|):  num = num + b*rho_q, den = den + b;  the result is num / den rounded to T.  A
 * poisoned pixel p is a quiet NaN (and never a neighbour).  rho is relative to the pixel's OWN sample count, so the mean may cross tile
 * borders; one |H_p| is an estimate with one degree of freedom, hence the mean (3 x 3 was chosen over 5 x 5 on the sweep of DESIGN.md 7.11).
 *
 * rtw_guided_filter_device_*: the device form of the filter above with one more input, `d_noise`: a DEVICE pointer, aligned to T, to
 * height*width elements (the map above, or any per-pixel relative noise the caller has).  rtw_denoise_t is unchanged and there is no flag
 * for it: the entry point is what makes the call guided.  Workspace, alignment, aliasing rules (d_noise is an input) and refusals are
 * those of the device form above; a null d_noise -> -1.  The definition differs from the one above in two places:
 *   Prepare.  valid(p) additionally needs a finite noise[p] = rho.  L = (e[0] + e[1]) + e[2];  s = rho * max(L, T(2^-6));
 *       v_p = min(max(s*s, V_MIN), V_MAX),  max(x, c) = x > c ? x : c,  min(x, c) = x < c ? x : c  (so a NaN s*s becomes V_MIN),
 *       V_MIN = 2^-40, V_MAX = 2^40: powers of two, normal numbers in binary32, so v_p is positive and finite and dc / v_p is never 0/0 or
 *       inf/inf.  v_p is kept for all levels.
 *   Level k.  The colour weight is  w_c = 1 / (1 + (dc / v_p)*inv_sc)  with the CENTRE pixel's v_p; inv_sc = T(1 / (sc*sc)), sc =
 *       sigma_color * 2^-k as above.  sigma_color thus counts estimated standard deviations of the pixel instead of colour units.
 * Everything else -- tap order, skipped taps, coverage, normal and depth terms, the end step -- is the definition above, bit for bit.
 *
 * rtw_accum_filtered_*: `out` is a HOST buffer of height*width*3 elements; blocking.  It runs, on the accumulator's device in a cached
 * context (the stream and buffer of the host forms), the resolve with gamma = 0 (per tile for an adaptive accumulator), the feature pass
 * rtw_accum_features_*, with guided = 1 the map rtw_accum_noise_* and the guided filter, with guided = 0 the filter above; d->gamma is
 * replaced by p->gamma and d->device by the accumulator's device; the result is copied to `out` once.  rtw_stats() afterwards reports
 * the feature pass's record.  Refusals, before any HIP call: nulls -> -1; guided other than 0 / 1 -> -2; everything rtw_accum_features_*
 * and the filter's own checks refuse; guided = 1 on a uniform accumulator -> -2.
 *   N accumulators in each launch: rtw_accum_*_batch_* below.  Out of scope: temporal reuse across views, device lists,
 * compact or sharded frames.  Additive to ABI 4: detected by symbol lookup. */
int rtw_accum_features_f32(rtw_scene_handle scene, const rtw_camera_f32 *cam, const rtw_params *p, rtw_accum_handle accum, void *d_out, void *hip_stream);
int rtw_accum_features_f64(rtw_scene_handle scene, const rtw_camera_f64 *cam, const rtw_params *p, rtw_accum_handle accum, void *d_out, void *hip_stream);
int rtw_accum_noise_f32(rtw_accum_handle accum, void *d_out, void *hip_stream);
int rtw_accum_noise_f64(rtw_accum_handle accum, void *d_out, void *hip_stream);
int rtw_guided_filter_device_f32(const rtw_denoise_t *d, int32_t width, int32_t height, const void *d_image, const void *d_features, const void *d_noise,
                                 void *d_out, void *d_work, void *hip_stream);
int rtw_guided_filter_device_f64(const rtw_denoise_t *d, int32_t width, int32_t height, const void *d_image, const void *d_features, const void *d_noise,
                                 void *d_out, void *d_work, void *hip_stream);
int rtw_accum_filtered_f32(rtw_scene_handle scene, const rtw_camera_f32 *cam, const rtw_params *p, const rtw_denoise_t *d, rtw_accum_handle accum, int32_t guided,
                           float *out);
int rtw_accum_filtered_f64(rtw_scene_handle scene, const rtw_camera_f64 *cam, const rtw_params *p, const rtw_denoise_t *d, rtw_accum_handle accum, int32_t guided,
                           double *out);

/* Batched feature and filter passes: N views of one scene, of one size, in each launch -- what rtw_render_batch_* is to the render.  A
 * turntable of N previews is then 2 + 1 + levels launches (render: views' upload + kernel; feature pass; prepare + levels) for any N,
 * instead of N times 2 + levels behind the one batched render.  No new arithmetic is defined:
 *   View v of a batched feature call is, bit for bit, rtw_render_features_* with cams[v] and seeds[v] (`seeds` == NULL: p->seed for every
 * view), in every scan mode, numerics mode and precision; view v writes W*H*8 elements at out + v*W*H*8.
 *   View v of a batched filter call is, bit for bit, the single-frame filter above (device or host form) on (image v, features v): images
 * and results hold the views one behind the other, view v at v*W*H*3 elements, the features at v*W*H*8; no tap ever reads another view.
 *   View v of rtw_render_filtered_batch_* is the render-and-denoise call above with cams[v] / seeds[v].
 *
 * rtw_render_features_batch_device_*: ONE launch; `d_out` is a DEVICE pointer, 16-byte aligned, to n_views*height*width*8 elements;
 * asynchronous like the single-view device form, the same render records: rtw_stats() afterwards reports samples = segments =
 * n_views*W*H*chunk_count, sphere_tests = segments * n, n_chunks = N, ONE kernel time.  rtw_render_features_batch_*: HOST buffers, blocking,
 * the cached per-device context of rtw_render_f32, one D2H.
 *   rtw_filter_batch_device_*: prepare + `levels` launches for all views, asynchronous on `hip_stream` of d->device.  The caller owns
 * `d_work`: n_views times the bytes the work-bytes call above returns for ONE frame, 16-byte aligned; its four planes (E, E', G, A) are
 * batch-major -- each holds n_views*W*H slots of 4 elements, view v at slot offset v*W*H --, so it is NOT n_views single-frame workspaces
 * side by side.  Alignment and aliasing rules are those of the single-frame device form, applied to the whole batch's extents.
 * rtw_filter_batch_*: HOST buffers, blocking, a leased context like the single-frame host form.  Neither changes what rtw_stats() reports.
 *   rtw_render_filtered_batch_*: the batched render of `p` with gamma = 0, the batched feature pass over all N effective chunks and the
 * batched filter with d->gamma replaced by p->gamma (d->device by p->device), in one device buffer on the cached context's stream; `out`
 * (HOST, n_views*height*width*3 elements) is written by one D2H; rtw_stats() afterwards reports the render's record.
 *   Refusals, all before any HIP call and before a handle is looked at.  Feature calls: the rules of rtw_render_batch_* together with
 * those of the feature pass -- null scene / cams / p / output -> -1; n_views < 1 -> -2; everything either refuses for `p`, the chunk range,
 * a misaligned d_out -> -2; a batch whose jobs the render's queues cannot number (which bounds the tiles of the feature launch too) -> -5.
 * Filter calls: nulls -> -1; everything the single-frame filter refuses, n_views < 1 -> -2; a batch of 2^39 pixels or more -> -5.
 * rtw_render_filtered_batch_*: both sets.  Then: a scene handle of the other precision -> -4.
 *   Accumulators as the input of a batch (the tiled feature pass, the noise-guided filter): the block behind these declarations.  Out of
 * scope: device lists.  History reuse across the views: rtw_render_sequence_* (the rtw_temporal_* block further down).
 * Additive to ABI 4: detected by symbol lookup. */
int rtw_render_features_batch_device_f32(rtw_scene_handle scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds,
                                         const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, void *d_out, void *hip_stream);
int rtw_render_features_batch_device_f64(rtw_scene_handle scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds,
                                         const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, void *d_out, void *hip_stream);
int rtw_render_features_batch_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds,
                                  const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, float *out);
int rtw_render_features_batch_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds,
                                  const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, double *out);
int rtw_filter_batch_device_f32(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views, const void *d_images,
                                const void *d_features, void *d_out, void *d_work, void *hip_stream);
int rtw_filter_batch_device_f64(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views, const void *d_images,
                                const void *d_features, void *d_out, void *d_work, void *hip_stream);
int rtw_filter_batch_f32(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views, const float *images, const float *features,
                         float *out);
int rtw_filter_batch_f64(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views, const double *images, const double *features,
                         double *out);
int rtw_render_filtered_batch_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds,
                                  const rtw_params *p, const rtw_denoise_t *d, float *out);
int rtw_render_filtered_batch_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds,
                                  const rtw_params *p, const rtw_denoise_t *d, double *out);

/* Batched passes over accumulators: the N accumulators a batched progressive or adaptive render (rtw_render_accum_batch_*,
 * rtw_render_adaptive_batch_*) filled go through ONE resolve launch, ONE feature launch, ONE noise launch and prepare + `levels` filter
 * launches -- 4 + levels launches and one D2H for any N, instead of N times that.  `accums`, `cams` and `seeds` are HOST arrays of n_views
 * entries as in rtw_render_accum_batch_* (`seeds` == NULL: p->seed for every view).  No new arithmetic is defined:
 *   View v of each call equals, bit for bit, the single-view entry point -- rtw_accum_resolve_*, rtw_accum_features_*, rtw_accum_noise_*,
 * rtw_guided_filter_device_*, rtw_accum_filtered_* -- called with accums[v], cams[v], seeds[v].
 *   Layouts.  Frames are view-major: view v at v*W*H*3 elements (images), v*W*H*8 (features), v*W*H (noise maps).  The filter's workspace is
 * n_views times the single-frame bytes and batch-major, as rtw_filter_batch_device_* defines it; the guided form keeps v_p in the A plane's
 * fourth slot.
 *   Every call is asynchronous on `hip_stream` except rtw_accum_filtered_batch_*, which is blocking with one D2H (`out`: a HOST buffer of
 * n_views*height*width*3 elements; the cached context of the accumulators' device, as rtw_accum_filtered_*).  Every call only reads the
 * accumulators; it waits for EVERY accumulator's event and records it on every one afterwards, like a batched pass.  The resolve and the
 * noise call read a small device table of the views that is kept with accums[0]: a call whose table is the one staged last (the same
 * accumulators in the same order, holding the same samples -- a resolve followed by the noise map, a batch read again) enqueues and returns;
 * a call with ANOTHER table first waits on the host until the copy of the previous one has left its staging buffer, i.e. until the work
 * queued in front of that copy has run.
 *   rtw_stats() after rtw_accum_features_batch_* and after rtw_accum_filtered_batch_* reports the ONE feature launch: samples = segments =
 * the sum over views and tiles of valid pixels x chunks held, ONE kernel time.  The other calls leave rtw_stats() alone.
 *   rtw_accum_features_batch_* takes accumulators that are all adaptive -- every one settled; the feature kernel's tiled batched instance
 * reads C_t of tile t of view v from the view's own device array -- or all uniform: each holds exactly one chunk interval and it is the SAME
 * [b, b + C) in every view, the batched feature pass above runs over it.  A mix of the two kinds, or uniform accumulators with different
 * intervals -> -2.  rtw_accum_resolve_batch_* takes either kind in any mix.
 *   Refusals, all before any HIP call and with no accumulator touched.  Nulls, including a null entry of `accums` -> -1.  n_views < 1; one
 * accumulator given twice; everything the single-view call refuses for `p`, `d`, alignment or aliasing (applied to the batch's extents);
 * guided other than 0 / 1; guided = 1 or a noise call on a uniform accumulator; an accumulator that holds nothing; an adaptive one whose
 * last adaptive call did not finish -> -2.  An accumulator of another size, device or precision; one not bound to (cams[v], seeds[v], p);
 * for the noise call, accumulators whose spp, chunk size or dark_floor differ from accums[0]'s (the kernel takes one set) -> -4.  A batch
 * the feature launch's tile numbering or the filter's 2^39-pixel rule cannot hold -> -5; rtw_accum_resolve_batch_*, whose one launch numbers
 * three elements per pixel: n_views * width * height >= 2^37 -> -5.
 *   Out of scope: temporal reuse across the views, device lists, compact or sharded frames.  Additive to ABI 4:
 * detected by symbol lookup. */
int rtw_accum_resolve_batch_f32(const rtw_accum_handle *accums, int32_t n_views, int32_t gamma, void *d_out, void *hip_stream);
int rtw_accum_resolve_batch_f64(const rtw_accum_handle *accums, int32_t n_views, int32_t gamma, void *d_out, void *hip_stream);
int rtw_accum_features_batch_f32(rtw_scene_handle scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p,
                                 const rtw_accum_handle *accums, void *d_out, void *hip_stream);
int rtw_accum_features_batch_f64(rtw_scene_handle scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p,
                                 const rtw_accum_handle *accums, void *d_out, void *hip_stream);
int rtw_accum_noise_batch_f32(const rtw_accum_handle *accums, int32_t n_views, void *d_out, void *hip_stream);
int rtw_accum_noise_batch_f64(const rtw_accum_handle *accums, int32_t n_views, void *d_out, void *hip_stream);
int rtw_guided_filter_batch_device_f32(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views, const void *d_images,
                                       const void *d_features, const void *d_noise, void *d_out, void *d_work, void *hip_stream);
int rtw_guided_filter_batch_device_f64(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views, const void *d_images,
                                       const void *d_features, const void *d_noise, void *d_out, void *d_work, void *hip_stream);
int rtw_accum_filtered_batch_f32(rtw_scene_handle scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p,
                                 const rtw_denoise_t *d, const rtw_accum_handle *accums, int32_t guided, float *out);
int rtw_accum_filtered_batch_f64(rtw_scene_handle scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p,
                                 const rtw_denoise_t *d, const rtw_accum_handle *accums, int32_t guided, double *out);

/* Feature-guided upsampler: a full-size image from a small render, guided by a full-size feature pass.  A feature pass traces one primary
 * scan per pixel and chunk, a render about 2.7 segments per sample: a frame path-traced at half width (a quarter of the samples) takes
 * its silhouettes, normals and albedo detail from the feature buffers of the full frame.
 *
 * The definition.  Everything is computed in the element type T (binary32 or binary64); every operation is rounded once, no FMA, no
 * reassociation; quotients and the final sqrt are the correctly rounded IEEE ones; subnormals are kept, as in the denoiser.
 *   Inputs.  The small frame is w x h: `image_lo` (h*w*3, normally a gamma = 0 image) and `features_lo` (h*w*8).  The full frame is W x H:
 * `features_hi` (H*W*8); the result holds H*W*3 elements.  Layouts are those of the render and feature entry points: pixel (i, j) (0-based
 * row, column) at j*rows + i.  1 <= w <= W and 1 <= h <= H.
 *   Small frame.  It is prepared exactly as the denoiser above prepares a frame: valid(q), has(q), n_q, z_q, cov_q, a_q and e_q (with
 * RTW_UPSAMPLE_DEMODULATE a = max(f, T(2^-6)) and e = c / a, otherwise a = 1 and e = c).  Then `levels` (0..8) passes of the denoiser's level
 * definition run on e at the small size, with the steps 2^k and the same inv_sc(k) and inv_sz; no pass is a final one -- nothing is
 * multiplied back and no gamma is applied.  With levels = 0, e is prepare's e.
 *   Full-size pixel P = (i, j), its feature slots F[0..7].  valid(P): all eight are finite.  cov_P = F[7]; has(P) = valid(P) and cov_P > 0.
 * If has(P): n_P = F[3..5] / cov_P and z_P = F[6] / cov_P, otherwise both are 0.  a_P[k] = max(F[k], T(2^-6)) with
 * RTW_UPSAMPLE_DEMODULATE, else 1.
 *   Position in the small frame (pixel centres coincide), in exact integers:  num_x = (2j + 3)*w - 3W;  x0 = floor(num_x / 2W);
 * r_x = num_x - x0*2W, in [0, 2W);  fx = T(r_x) / T(2W) -- each conversion rounded to nearest even, one quotient.  Rows likewise: (i, h, H)
 * give y0 and fy.  x0 lies in [-2, w-1], and every full-size pixel has a tap inside the small frame with a positive spatial weight
 * (tests/test_upsample_ref.py checks both for every 1 <= w <= W <= 64): that is why w > W is refused.
 *   Taps.  16 of them: the column offset b = -1..2 is the outer, the row offset a = -1..2 the inner loop; the tap is q = (y0 + a, x0 + b).
 * kx = 1 - |T(b) - fx| * T(0.5), ky likewise with a and fy (each subtraction rounded once, the product by 0.5 exact, both >= 0); s = ky*kx.
 * A tap outside the small frame, or whose q is not valid, is skipped.  Any other tap:
 *       da[k] = a_P[k] - a_q[k];  dA = (da0*da0 + da1*da1) + da2*da2;  w_a = 1 / (1 + dA*inv_sa)
 *       t_v = 1 - |cov_P - cov_q|;  w_v = t_v > 0 ? t_v : +0
 *       w = (s*w_a)*w_v
 *       if has(P) and has(q):
 *           dot = (n_P.x*n_q.x + n_P.y*n_q.y) + n_P.z*n_q.z;  t = dot > 0 ? dot : +0, then t = t*t repeated m = normal_power_log2 times
 *           zs = z_P + z_q;  r = (z_P - z_q) / (zs > 0 ? zs : 1);  w_z = 1 / (1 + (r*r)*inv_sz)
 *           w = (w*t)*w_z
 *       sum_w = sum_w + w;  sum_e[k] = sum_e[k] + w*e_q[k];  sum_s = sum_s + s;  sum_se[k] = sum_se[k] + s*e_q[k]
 * All four sums start at +0.  inv_sa = T(1.0 / (sigma_albedo*sigma_albedo)), computed by the host in binary64.
 *   End.  If sum_w > 0: e[k] = sum_e[k] / sum_w.  Otherwise, if sum_s > 0: e[k] = sum_se[k] / sum_s -- the purely spatial fallback: every
 * guide rejected every tap.  Otherwise the pixel is not valid.  out[k] = e[k] * a_P[k] with RTW_UPSAMPLE_DEMODULATE, else e[k]; then sqrt per
 * channel if gamma = 1.  A pixel that is not valid, or whose valid(P) is false, is a quiet NaN in all three channels.  Without
 * RTW_UPSAMPLE_DEMODULATE a = 1 on both sides, so dA = 0 and w_a = 1 exactly: there is no special case.  (tests/upsample_ref.py restates all
 * of this on the CPU and the device agrees on the bits.)
 *
 * The device forms are asynchronous on `hip_stream` of the device u->device (-1: the current one).  The caller owns `d_work`: the bytes the
 * work-bytes call below returns for the SMALL frame (the denoiser's), times n_views for a batch, 16-byte aligned; no device workspace is
 * shared, so any number of calls may be in flight with a workspace each.  Both feature buffers are 16-byte aligned, the images aligned
 * to T; `d_out` aliases nothing, the workspace aliases no input.  Launches: prepare + `levels` + 1, for any number of views.
 *   Batches are batch-major as rtw_filter_batch_device_* defines it: view v's planes follow view v-1's, each at its own frame size -- the
 * small images at v*w*h*3 elements, the small features at v*w*h*8, the full features at v*W*H*8, the results at v*W*H*3; view v is, bit
 * for bit, the single call on its frames.
 *   The host forms are blocking, lease a cached context like rtw_denoise_f32 and copy the result back once.  Neither the host nor the device
 * forms change what rtw_stats() reports.
 *   The render-and-upsample call: let q = *p with the small width and height and gamma 0.  It renders q, runs the feature pass over all
 * N_q effective chunks of q, runs the feature pass of `p` at full size over the chunks [0, hi_chunks) (hi_chunks = 0: all N_p), and
 * upsamples with u->gamma replaced by p->gamma and u->device by p->device -- all on the cached context's stream, with one D2H of the
 * full-size result: 5 + `levels` launches for any number of views.  rtw_stats() afterwards reports the small render's record.
 *   Refusals, all decided before any HIP call: a null argument -> -1; levels outside 0..8, normal_power_log2 outside 0..7, unknown flag
 * bits, gamma other than 0 or 1, device < -1, hi_chunks < 0, a sigma that is not finite and positive (sigma_color also with levels = 0),
 * a width or height < 1, a small frame larger than the full one in either direction, misaligned or aliasing pointers, elem_bytes other
 * than 4 or 8, n_views < 1 -> -2; hi_chunks beyond N_p -> -2; a full frame of 2^31 8x8 tiles or more, a batch of 2^39 full-size pixels
 * or more -> -5; the render calls additionally refuse everything a feature render of `p` and of q refuses.  Out of scope (DESIGN.md
 * section 9): accumulators as the input, a noise-guided form, device lists, an LDS-tiled kernel.  Additive to ABI 4: detected by symbol lookup. */
#define RTW_UPSAMPLE_DEMODULATE 1  /* filter and interpolate image / albedo, multiply the full-size albedo back at the end */
typedef struct {
    int32_t levels;             /* 0..8 a-trous passes at the small size before the upsampling */
    int32_t normal_power_log2;  /* 0..7: m, normal weight = max(0, n.n')^(2^m) */
    int32_t flags;              /* RTW_UPSAMPLE_* */
    int32_t gamma;              /* 1 = sqrt per channel at the end, 0 = linear */
    int32_t device;             /* -1 = current */
    int32_t hi_chunks;          /* render-and-upsample calls: chunks [0, hi_chunks) of the full-size feature pass; 0 = all N; >= 0 everywhere */
    double  sigma_color;        /* the levels' colour sigma; > 0, finite (validated even with levels = 0) */
    double  sigma_depth;        /* levels and taps; > 0, finite */
    double  sigma_albedo;       /* taps; > 0, finite */
} rtw_upsample_t;               /* 48 bytes */
int64_t rtw_upsample_work_bytes(int32_t lo_width, int32_t lo_height, int32_t elem_bytes);
int rtw_upsample_device_f32(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, const void *d_image_lo,
                            const void *d_features_lo, const void *d_features_hi, void *d_out, void *d_work, void *hip_stream);
int rtw_upsample_device_f64(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, const void *d_image_lo,
                            const void *d_features_lo, const void *d_features_hi, void *d_out, void *d_work, void *hip_stream);
int rtw_upsample_f32(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, const float *image_lo,
                     const float *features_lo, const float *features_hi, float *out);
int rtw_upsample_f64(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, const double *image_lo,
                     const double *features_lo, const double *features_hi, double *out);
int rtw_upsample_batch_device_f32(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, int32_t n_views,
                                  const void *d_images_lo, const void *d_features_lo, const void *d_features_hi, void *d_out, void *d_work, void *hip_stream);
int rtw_upsample_batch_device_f64(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, int32_t n_views,
                                  const void *d_images_lo, const void *d_features_lo, const void *d_features_hi, void *d_out, void *d_work, void *hip_stream);
int rtw_upsample_batch_f32(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, int32_t n_views,
                           const float *images_lo, const float *features_lo, const float *features_hi, float *out);
int rtw_upsample_batch_f64(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, int32_t n_views,
                           const double *images_lo, const double *features_lo, const double *features_hi, double *out);
int rtw_render_upsampled_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cam, const rtw_params *p, int32_t lo_width, int32_t lo_height,
                             const rtw_upsample_t *u, float *out);
int rtw_render_upsampled_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cam, const rtw_params *p, int32_t lo_width, int32_t lo_height,
                             const rtw_upsample_t *u, double *out);
int rtw_render_upsampled_batch_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p,
                                   int32_t lo_width, int32_t lo_height, const rtw_upsample_t *u, float *out);
int rtw_render_upsampled_batch_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p,
                                   int32_t lo_width, int32_t lo_height, const rtw_upsample_t *u, double *out);

/* Temporal reprojection: history reuse along a camera path.  N cameras along a path over one static scene at 1-4 spp each see mostly what
 * the previous camera saw: a temporal step blends a frame with the accumulated history of the previous frame, gathered where the pixel's
 * first-hit point lay in the previous view.  One new kernel, a small state, and the host paths; everything else (the linear image, the
 * feature buffers) is what the passes above leave in HBM.
 *
 * The definition.  Everything is computed in the element type T (binary32 or binary64); every operation is rounded once, no FMA, no
 * reassociation; quotients and sqrt are the correctly rounded IEEE ones; subnormals are kept; weights are rational; a tap that does not take
 * part is dropped by a select, never by a zero weight.  A temporal step takes the parameters rtw_temporal_t, the current camera `cam` and
 * the previous one `cam_prev`, the current linear image (H*W*3, the render entry points' layout, normally gamma = 0), the current features
 * (H*W*8, the feature entry points' layout) and the previous STATE, which may be absent (the first frame: then cam_prev is absent too);
 * it produces an image (H*W*3) and the next state.  Pixel (i, j) (0-based row, column) is slot p = j*H + i.
 *   State.  Three planes, one behind the other, each starting on a 16-byte boundary: E = (e0, e1, e2, z), a 4-element slot per pixel, at
 * byte 0; G = (n.x, n.y, n.z, cov), a 4-element slot per pixel, at byte 4*W*H*sizeof(T) -- cov = NaN marks a pixel that is not valid --;
 * L = len, one element per pixel, at byte 8*W*H*sizeof(T).  rtw_temporal_state_bytes returns the size: 9*W*H elements rounded up to a
 * multiple of 16 bytes (monotone in the size; < 0: an error code).  The layout is public.
 *   Prepare, per pixel, exactly the denoiser's: valid = all 3 + 8 inputs are finite; cov = f[7]; has = valid and cov > 0; if has:
 * n = f[3..5] / cov (three quotients) and z = f[6] / cov, otherwise n = 0 and z = 0.  With RTW_TEMPORAL_DEMODULATE a[k] = max(f[k], T(2^-6))
 * and e[k] = c[k] / a[k], otherwise a = 1 and e = c.
 *   The pixel's own ray in the current camera.  The trace kernel samples column j at (j+1)/W + [0,1)/W and rows likewise; the centre of
 * those samples is  su = (T(j) + T(1.5)) / T(W),  tv = (T(H - i) - T(0.5)) / T(H)  (integers converted to T, one quotient each).  Per
 * component  D = ((llc + su*hor) + tv*ver) - origin;  l2 = (D.x*D.x + D.y*D.y) + D.z*D.z;  nD = D / sqrt(l2) (three quotients by the one
 * square root).  The lens is ignored: a stated approximation (lens_radius is not read).
 *   The point to reproject, relative to the previous origin.  If has: Pw = origin + z*nD and d = Pw - origin_prev (per component, in this
 * order).  Else, for a sky pixel, the point at infinity: d = nD.
 *   Projection into the previous camera.  The host computes in binary64 from the previous camera's fields (converted to binary64 exactly):
 * q = llc - origin, Kw = q.w, Qh = q.hor, Qv = q.ver, ih = 1/(hor.hor), iv = 1/(ver.ver), and rounds each to T once; likewise
 * inv_sz = T(1/(sigma_depth*sigma_depth)), w_min = T(min_weight), n_max = T(history_max).  Every three-term dot product, on the host and on
 * the device, is grouped (x + y) + z.  The device computes
 *       dw = d.w_prev;  front = dw < 0;  lam = Kw / dw
 *       s = (lam*(d.hor_prev) - Qh)*ih;  t = (lam*(d.ver_prev) - Qv)*iv
 *       x = s*T(W) - T(1.5);  y = (T(H) - T(0.5)) - t*T(H)
 *       inr = x > -1 and x < W and y > -1 and y < H   (a NaN fails)
 *       x0 = floor(x), fx = x - T(x0);  y0 = floor(y), fy = y - T(y0)
 * A position with inr false decides nothing (the pixel resets below), so x0, fx, y0, fy are only defined under inr.  The depth the point
 * is expected to have in the previous view is zexp = sqrt((d.x*d.x + d.y*d.y) + d.z*d.z), used for has pixels only.
 *   Taps.  b = 0, 1 is the outer and c = 0, 1 the inner loop; the tap pixel q is column x0 + b, row y0 + c; kx = b ? fx : 1 - fx,
 * ky = c ? fy : 1 - fy, sb = ky*kx.  A tap outside the frame, or whose state slot is not valid (G.w is NaN), is skipped.  Any other tap:
 *       t_v = 1 - |cov_p - cov_q|;  w_v = t_v > 0 ? t_v : +0
 *       w = sb*w_v
 *       if has(p) and cov_q > 0:
 *           dot = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z;  t = dot > 0 ? dot : +0, then t = t*t repeated m = normal_power_log2 times
 *           zs = zexp + z_q;  r = (zexp - z_q) / (zs > 0 ? zs : 1);  w_z = 1 / (1 + (r*r)*inv_sz)
 *           w = (w*t)*w_z
 *       sum_w = sum_w + w;  sum_e[k] = sum_e[k] + w*e_q[k];  sum_l = sum_l + w*len_q
 * All sums start at +0; n_q, z_q, cov_q, e_q and len_q are the state's.
 *   Blend.  accept = the previous state is present and front and inr and sum_w >= w_min (a NaN fails).  If accepted:
 *       eh[k] = sum_e[k] / sum_w;  lh = sum_l / sum_w;  l1 = lh + 1;  n' = l1 < n_max ? l1 : n_max;  alpha = 1 / n'
 *       e'[k] = eh[k] + alpha*(e[k] - eh[k]);  len' = n'
 * Otherwise the pixel RESETS: e' = e and len' = 1.
 *   End.  out[k] = e'[k]*a[k] with RTW_TEMPORAL_DEMODULATE, else e'[k]; then sqrt per channel if gamma = 1.  The next state is E = (e', z),
 * G = (n, cov), L = len'.  A pixel that is not valid is a quiet NaN in all three `out` channels, has G.w = NaN and zeros in the rest of its
 * state; it is never a tap.  (tests/temporal_ref.py restates all of this on the CPU and the device agrees on the bits.)
 *
 * rtw_temporal_device_*: asynchronous on `hip_stream` of the device t->device (-1: the current one); rtw_stats() is left alone.
 * d_state_prev == NULL together with cam_prev == NULL is the first frame: every pixel resets.  `d_features` and both states are 16-byte
 * aligned, `d_image` and `d_out` aligned to T; `d_out` and `d_state_next` alias neither each other nor any input.  One launch.
 *   rtw_temporal_*: the host-buffer form, blocking, through the cached per-device context like rtw_denoise_f32; `state_prev` (with
 * `cam_prev`) may be NULL: the first frame; `state_next` receives rtw_temporal_state_bytes bytes.  rtw_stats() is left alone.
 *   rtw_render_sequence_*: n_views cameras along a path, all on the cached context's stream -- one batched render of `p` with gamma = 0,
 * one batched feature pass over all N effective chunks, n_views temporal steps in view order (view 0 is the first frame, view v uses
 * cams[v-1] and the state view v-1 left; two states ping-pong), and, if `d` is not NULL, one batched filter pass (rtw_filter_batch_*'s
 * launch sequence) over the n_views accumulated LINEAR images and their features -- then one D2H of n_views*H*W*3 elements.  p->gamma is
 * applied exactly once, by the last stage that runs: with `d` the steps run with gamma = 0 and the filter with p->gamma, without it the steps
 * run with p->gamma (t->gamma and d->gamma are replaced, t->device and d->device by p->device).  `seeds`: n_views of them, or NULL (p->seed).
 * View v equals, bit for bit, the chain of the single calls.  rtw_stats() afterwards reports the render's record.
 *   Refusals, all decided before any HIP call: a null argument -> -1; unknown flag bits, gamma other than 0 or 1, reserved != 0,
 * device < -1, normal_power_log2 outside 0..7, a sigma_depth that is not finite and positive, min_weight outside (0, 1], history_max not
 * finite or < 1, width or height < 1, elem_bytes other than 4 or 8, misaligned or aliasing pointers, exactly one of cam_prev /
 * d_state_prev (state_prev) null -> -2; a frame of 2^31 8x8 tiles or more (the denoiser's frame rule) -> -5; the sequence call additionally
 * refuses everything rtw_render_filtered_batch_* refuses for its arguments (with `d` NULL: everything a batched feature render refuses).
 *   Left out on purpose: accumulators or the upsampler as the step's input,
 * device lists, a variance-guided alpha.  (Spheres that move between the frames: the rtw_first_hit_motion_* block further down; the steps of
 * this block know no motion but the camera's.)
 * (Neighbourhood colour clamping: the rtw_clamped_step_* block further down.  A per-pixel noise map from the history's second moments, and the sequence call that feeds it to the
 * noise-guided filter: the block behind these declarations.)  Additive to ABI 4: detected by symbol lookup. */
#define RTW_TEMPORAL_DEMODULATE 1  /* accumulate image / albedo, multiply the current albedo back at the end */
typedef struct {
    int32_t normal_power_log2;  /* 0..7: m, normal weight = max(0, n.n')^(2^m) */
    int32_t flags;              /* RTW_TEMPORAL_* */
    int32_t gamma;              /* 1 = sqrt per channel at the end, 0 = linear */
    int32_t device;             /* -1 = current */
    int32_t reserved[2];        /* 0 */
    double  sigma_depth;        /* > 0, finite */
    double  min_weight;         /* in (0, 1]: the least sum of tap weights a history is accepted with */
    double  history_max;        /* >= 1, finite: where len saturates (alpha never falls below 1 / history_max) */
} rtw_temporal_t;               /* 48 bytes */
int64_t rtw_temporal_state_bytes(int32_t width, int32_t height, int32_t elem_bytes);
int rtw_temporal_device_f32(const rtw_temporal_t *t, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width, int32_t height,
                            const void *d_image, const void *d_features, const void *d_state_prev, void *d_state_next, void *d_out, void *hip_stream);
int rtw_temporal_device_f64(const rtw_temporal_t *t, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width, int32_t height,
                            const void *d_image, const void *d_features, const void *d_state_prev, void *d_state_next, void *d_out, void *hip_stream);
int rtw_temporal_f32(const rtw_temporal_t *t, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width, int32_t height,
                     const float *image, const float *features, const void *state_prev, void *state_next, float *out);
int rtw_temporal_f64(const rtw_temporal_t *t, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width, int32_t height,
                     const double *image, const double *features, const void *state_prev, void *state_next, double *out);
int rtw_render_sequence_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p,
                            const rtw_temporal_t *t, const rtw_denoise_t *d /* may be NULL */, float *out);
int rtw_render_sequence_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p,
                            const rtw_temporal_t *t, const rtw_denoise_t *d /* may be NULL */, double *out);

/* Temporal moments: a per-pixel noise estimate from the history, for the noise-guided filter (rtw_guided_filter_device_*,
 * rtw_guided_filter_batch_device_*).  A pixel with a long history has seen many independent samples of its radiance, a pixel that has just
 * been disoccluded one; the step above can carry the second moment of what it accumulates, and a second pass turns state and moments into
 * the relative-noise map the guided filter already takes.  Where the history is short a spatial estimate stands in.  Nothing above changes:
 * the 9-element state keeps its layout and size, the moments live in a buffer of their own, and the step's image and state are the same bits.
 * (The entry points are named rtw_history_* and rtw_render_path_guided_*: the names of the block above are a closed set.)
 *
 * The definition, in the arithmetic of the block above (T, one rounding per operation, no FMA, IEEE quotients and sqrt, rational weights,
 * a tap that takes no part is dropped by a select).
 *   Moment plane.  M holds one element per pixel at slot p = j*H + i: the running second moment of the pixel's (de)modulated luminance; a
 * pixel that is not valid stores 0.  rtw_history_moment_bytes returns its size: W*H elements rounded up to a multiple of 16 bytes (the error
 * codes are those of rtw_temporal_state_bytes).
 *   Step with moments.  rtw_temporal_device_* with two more pointers, the previous and the next moment plane.  The image and all three state
 * planes are those of rtw_temporal_device_* on the bits.  In addition, with e the pixel's (de)modulated colour of Prepare:
 *       y = (e[0] + e[1]) + e[2];  y2 = y*y
 * every tap that contributes (the same taps, the same w, the same order) adds  sum_m = sum_m + w*M_q  (sum_m starts at +0), and
 *       accepted:  mh = sum_m / sum_w;  M' = mh + alpha*(y2 - mh)          reset, or the first frame:  M' = y2
 * M' is stored for a valid pixel, 0 for any other.
 *   Noise map.  A second pass over the NEXT state (E, G, L) and its moment plane M; `d_noise` receives height*width elements, pixel (i, j) at
 * j*height + i (the layout rtw_guided_filter_device_* reads).  A pixel whose slot is not valid (G.w is NaN) is a quiet NaN.  Any other pixel p,
 * with inv_sz = T(1/(sigma_depth*sigma_depth)) and ml = T(min_len) rounded on the host as above, m = normal_power_log2, r = radius:
 *       Lm = (E[0] + E[1]) + E[2];  vt = M - Lm*Lm;  var = vt > 0 ? vt : +0
 *       if not (len >= ml), the spatial estimate: S0 = S1 = S2 = +0; dj = -r..r is the outer and di = -r..r the inner loop; the tap q is row
 *       i + di, column j + dj; a tap outside the frame or whose slot is not valid is skipped; any other tap (the centre among them):
 *           t_v = 1 - |cov_p - cov_q|;  w = t_v > 0 ? t_v : +0                                   (the step's tap weight with sb = 1)
 *           if cov_p > 0 and cov_q > 0:
 *               dot = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z;  t = dot > 0 ? dot : +0, then t = t*t repeated m times
 *               zs = z_p + z_q;  rz = (z_p - z_q) / (zs > 0 ? zs : 1);  w_z = 1 / (1 + (rz*rz)*inv_sz)          (zexp = z_p)
 *               w = (w*t)*w_z
 *           Lm_q = (E_q[0] + E_q[1]) + E_q[2];  S0 = S0 + w;  S1 = S1 + w*Lm_q;  S2 = S2 + w*M_q
 *       then  mu = S1 / S0;  vs = S2 / S0 - mu*mu;  var = vs > 0 ? vs : +0
 *       v = var / len;  rho = sqrt(v) / (Lm > T(2^-6) ? Lm : T(2^-6))
 * The centre tap has t_v = 1, so S0 > 0 unless a covered pixel's normal is the zero vector (then 0 / 0: the map is NaN there, which the
 * guided filter treats as a pixel that is not valid).  rho is relative to the luminance of the accumulated, (de)modulated colour: the
 * guided filter's prepare multiplies it back when it runs with the same demodulation as the step.  (tests/temporal_noise_ref.py restates
 * all of this on the CPU, twice, and the device agrees on the bits.)
 *
 * rtw_history_moments_device_*: rtw_temporal_device_* with `d_moment_prev` / `d_moment_next`, DEVICE pointers to rtw_history_moment_bytes
 * bytes, 16-byte aligned; d_moment_prev is NULL exactly when d_state_prev is; the three outputs alias neither each other nor an input.  One
 * launch, asynchronous.
 *   rtw_history_noise_device_*: the map of `d_state` and `d_moment` into `d_noise` (aligned to T, aliasing neither input), one launch,
 * asynchronous on `hip_stream` of the device n->device (-1: the current one).
 *   rtw_history_moments_*: the host-buffer form, blocking, through the cached context like rtw_temporal_f32: the step, then the map of what
 * it left; `state_prev`, `moment_prev` and `cam_prev` are NULL together (the first frame); it returns the image, the next state, the next
 * moment plane and the noise map (n->device is replaced by t->device).  rtw_stats() is left alone.
 *   rtw_render_path_guided_*: rtw_render_sequence_* with `d` required.  The steps are the steps with moments; after step v one noise
 * launch writes view v of an N-view noise region (before the ping-pong reuses that state: stream order); then ONE noise-guided batched
 * filter pass (rtw_guided_filter_batch_device_*'s launch sequence) over the N accumulated LINEAR images, their features and the N maps;
 * one D2H.  p->gamma is applied once, by the filter.  View v equals the chain of the single device calls on the bits; rtw_stats() reports
 * the render's record.
 *   Refusals, all decided before any HIP call: a null argument -> -1; everything rtw_temporal_device_* refuses, its alignment and aliasing
 * rules extended to the moment planes, exactly one of d_state_prev / d_moment_prev null -> -2; radius outside 1..3, normal_power_log2
 * outside 0..7, device < -1, reserved != 0, a sigma_depth that is not finite and positive, min_len not finite or < 1, a misaligned or
 * aliasing pointer -> -2; the frame rule -> -5; the sequence call refuses everything rtw_render_sequence_* refuses and, with -2, a `t` and
 * a `d` whose DEMODULATE flags differ (the map is relative to the state's luminance).
 *   The defaults (radius 2, normal_power_log2 1, sigma_depth 0.1, min_len 4) are UNTUNED beyond the record of DESIGN.md 7.19.  Left out on
 * purpose: a variance-driven alpha, smoothing of the map, moments for accumulators or
 * the upsampler, device lists, an LDS-tiled window.  Additive to ABI 4: detected by symbol lookup. */
typedef struct {
    int32_t radius;             /* 1..3: the spatial estimate's window is (2*radius + 1)^2 */
    int32_t normal_power_log2;  /* 0..7: m of the window's normal weight */
    int32_t device;             /* -1 = current */
    int32_t reserved[3];        /* 0 */
    double  sigma_depth;        /* > 0, finite: the window's relative-depth weight */
    double  min_len;            /* >= 1, finite: a history at least this long uses its own moments */
} rtw_temporal_noise_t;         /* 40 bytes */
int64_t rtw_history_moment_bytes(int32_t width, int32_t height, int32_t elem_bytes);
int rtw_history_moments_device_f32(const rtw_temporal_t *t, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width, int32_t height,
                                    const void *d_image, const void *d_features, const void *d_state_prev, const void *d_moment_prev, void *d_state_next,
                                    void *d_moment_next, void *d_out, void *hip_stream);
int rtw_history_moments_device_f64(const rtw_temporal_t *t, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width, int32_t height,
                                    const void *d_image, const void *d_features, const void *d_state_prev, const void *d_moment_prev, void *d_state_next,
                                    void *d_moment_next, void *d_out, void *hip_stream);
int rtw_history_noise_device_f32(const rtw_temporal_noise_t *n, int32_t width, int32_t height, const void *d_state, const void *d_moment, void *d_noise,
                                  void *hip_stream);
int rtw_history_noise_device_f64(const rtw_temporal_noise_t *n, int32_t width, int32_t height, const void *d_state, const void *d_moment, void *d_noise,
                                  void *hip_stream);
int rtw_history_moments_f32(const rtw_temporal_t *t, const rtw_temporal_noise_t *n, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width,
                             int32_t height, const float *image, const float *features, const void *state_prev, const void *moment_prev, void *state_next,
                             void *moment_next, float *out, float *noise);
int rtw_history_moments_f64(const rtw_temporal_t *t, const rtw_temporal_noise_t *n, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width,
                             int32_t height, const double *image, const double *features, const void *state_prev, const void *moment_prev, void *state_next,
                             void *moment_next, double *out, double *noise);
int rtw_render_path_guided_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p,
                                   const rtw_temporal_t *t, const rtw_temporal_noise_t *n, const rtw_denoise_t *d, float *out);
int rtw_render_path_guided_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p,
                                   const rtw_temporal_t *t, const rtw_temporal_noise_t *n, const rtw_denoise_t *d, double *out);

/* Temporal clamp: neighbourhood colour clamping of the reprojected history.  The two blocks above trust a history completely once the
 * geometric tests accept it, and those tests see first-hit geometry only: what is view-dependent behind the first hit (a metal's reflection,
 * everything seen through a dielectric) and the blur of repeated bilinear resampling are reprojected as if painted on the surface, then
 * averaged for up to history_max frames.  The clamped step pulls the gathered history into mean +- sigma standard deviations of the CURRENT
 * frame's (2*radius + 1)^2 window before it blends, and can shorten the history it moved.  Nothing above changes: the step, the state, the
 * moment plane and every entry point of the two blocks above keep their bits and their layouts; this is one more form of the step.
 * (The entry points are named rtw_clamped_step_* and rtw_render_path_clamped_*: the names of the two blocks above are closed sets.)
 *
 * The definition, in the arithmetic of the temporal block (everything in T, one rounding per operation, no FMA, IEEE quotients and sqrt, a
 * tap that takes no part is dropped by a select).  The step is rtw_history_moments_device_*'s (rtw_temporal_device_*'s when no moment planes
 * are given) with one insertion between "Taps" and "Blend".  ks = T(sigma) and ls = T(len_scale) are rounded on the host.
 *   Window of the current frame.  r = radius; S0 = S1[k] = S2[k] = +0; dj = -r..r is the outer and di = -r..r the inner loop; the tap q is
 * row i + di, column j + dj.  A tap outside the frame, or whose pixel is not valid by Prepare (any of its 3 + 8 inputs not finite), is
 * skipped.  Any other tap (the centre among them), with e_q, n_q, z_q, cov_q those of Prepare for pixel q of the current frame:
 *       with RTW_CLAMP_GUIDES, the noise map's window weight on the current frame's guides (the step's tap weight with sb = 1, zexp = z_p;
 *       m = t->normal_power_log2 and inv_sz = T(1/(t->sigma_depth*t->sigma_depth)) are the step's):
 *           t_v = 1 - |cov_p - cov_q|;  w = t_v > 0 ? t_v : +0
 *           if has(p) and cov_q > 0:
 *               dot = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z;  t = dot > 0 ? dot : +0, then t = t*t repeated m times
 *               zs = z_p + z_q;  rz = (z_p - z_q) / (zs > 0 ? zs : 1);  w_z = 1 / (1 + (rz*rz)*inv_sz);  w = (w*t)*w_z
 *           S0 = S0 + w;  S1[k] = S1[k] + w*e_q[k];  S2[k] = S2[k] + w*(e_q[k]*e_q[k])
 *       without it w = 1 and the products by w are not formed:
 *           S0 = S0 + 1;  S1[k] = S1[k] + e_q[k];    S2[k] = S2[k] + e_q[k]*e_q[k]
 *   then per channel
 *       mu = S1/S0;  vt = S2/S0 - mu*mu;  var = vt > 0 ? vt : +0;  sd = sqrt(var);  lo = mu - ks*sd;  hi = mu + ks*sd
 *   Clamp.  With eh and lh the history of "Blend" (eh[k] = sum_e[k] / sum_w, lh = sum_l / sum_w):
 *       hc[k] = eh[k] < lo[k] ? lo[k] : (eh[k] > hi[k] ? hi[k] : eh[k])      (a NaN bound -- S0 = 0 -- fails both comparisons: hc = eh)
 *       moved = some channel has hc[k] != eh[k];  lh' = moved ? lh*ls : lh
 * and the blend continues with hc and lh' in place of eh and lh: l1 = lh' + 1; n' = l1 < n_max ? l1 : n_max; alpha = 1 / n';
 * e'[k] = hc[k] + alpha*(e[k] - hc[k]); len' = n'.  With moment planes mh = sum_m / sum_w is blended with the alpha that results,
 * M' = mh + alpha*(y2 - mh): the second moment itself is not clamped.
 *   Reset and first frame.  A pixel that resets, and the first frame, are the plain step's: the window decides nothing there (the first
 * frame runs the plain step's kernel).  A pixel that is not valid is the plain step's as well.
 *   Equivalence.  Where no pixel is moved the call equals rtw_temporal_device_* / rtw_history_moments_device_* on the bits: image, state and
 * moment plane.  (tests/temporal_clamp_ref.py restates all of this on the CPU, twice, and the device agrees on the bits.)
 *
 * rtw_clamped_step_device_*: rtw_history_moments_device_* with the clamp `c` behind `t`; d_moment_prev and d_moment_next are NULL together
 * (no moments: rtw_temporal_device_*'s step) or follow rtw_history_moments_device_*'s rule.  One launch, asynchronous; rtw_stats() is left alone.
 *   rtw_clamped_step_*: the host-buffer form, blocking, through the cached context like rtw_temporal_f32; `moment_prev` / `moment_next` are
 * optional in the same way; there is no noise map (rtw_history_noise_device_* reads the state and the plane this call returns).
 *   rtw_render_path_clamped_*: n_views cameras along a path with clamped steps.  `n` and `d` both NULL: rtw_render_sequence_* without a
 * filter; `d` alone: with the plain filter; `n` and `d`: rtw_render_path_guided_*; `n` without `d` -> -2.  In every case the steps behind
 * view 0 are clamped steps; view v equals the chain of the single device calls on the bits; rtw_stats() reports the render's record.
 *   Refusals, all decided before any HIP call: a null `c` (or any other null argument that is not optional) -> -1; radius outside 1..3,
 * unknown flag bits, reserved != 0, sigma not finite or < 0, len_scale outside [0, 1] or NaN -> -2; everything the underlying temporal,
 * moments or sequence call refuses, with that call's code.
 *   The defaults (radius 1, no flags, sigma 1, len_scale 1) are UNTUNED beyond the record of DESIGN.md 7.21.  Left out on purpose (DESIGN.md
 * section 9): a continuous variance-driven alpha, clamping in another colour space, clamping the second moment,
 * device lists.  Additive to ABI 4: detected by symbol lookup. */
#define RTW_CLAMP_GUIDES 1      /* weight the window's taps by the current frame's guides (coverage, normal, depth) */
typedef struct {
    int32_t radius;             /* 1..3: the window is (2*radius + 1)^2 */
    int32_t flags;              /* RTW_CLAMP_* */
    int32_t reserved[2];        /* 0 */
    double  sigma;              /* finite, >= 0: the bounds are mean -+ sigma standard deviations */
    double  len_scale;          /* in [0, 1]: the gathered history length of a pixel the clamp moved is multiplied by it */
} rtw_temporal_clamp_t;         /* 32 bytes */
int rtw_clamped_step_device_f32(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width,
                                    int32_t height, const void *d_image, const void *d_features, const void *d_state_prev, const void *d_moment_prev /* may be NULL */,
                                    void *d_state_next, void *d_moment_next /* may be NULL */, void *d_out, void *hip_stream);
int rtw_clamped_step_device_f64(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width,
                                    int32_t height, const void *d_image, const void *d_features, const void *d_state_prev, const void *d_moment_prev /* may be NULL */,
                                    void *d_state_next, void *d_moment_next /* may be NULL */, void *d_out, void *hip_stream);
int rtw_clamped_step_f32(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width,
                             int32_t height, const float *image, const float *features, const void *state_prev, const void *moment_prev /* may be NULL */,
                             void *state_next, void *moment_next /* may be NULL */, float *out);
int rtw_clamped_step_f64(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width,
                             int32_t height, const double *image, const double *features, const void *state_prev, const void *moment_prev /* may be NULL */,
                             void *state_next, void *moment_next /* may be NULL */, double *out);
int rtw_render_path_clamped_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p,
                                 const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, const rtw_temporal_noise_t *n /* may be NULL */,
                                 const rtw_denoise_t *d /* may be NULL */, float *out);
int rtw_render_path_clamped_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p,
                                 const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, const rtw_temporal_noise_t *n /* may be NULL */,
                                 const rtw_denoise_t *d /* may be NULL */, double *out);

/* Batched temporal steps: n_paths independent camera paths over one scene (a stereo pair, several orbiting cameras, candidate camera moves
 * side by side) advance in each launch.  At preview sizes a step is all launch cost; S paths share it.
 *
 * The definition.  There is no new arithmetic.  Path s of a batched step is, bit for bit, the single call for path s -- one of
 * rtw_temporal_device_*, rtw_history_moments_device_* or rtw_clamped_step_device_*, chosen by the pointer rule of rtw_clamped_step_device_*
 * extended by `c`: c == NULL is the plain step, both moment pointers NULL is the step without moments.  Path s of the batched noise map is
 * rtw_history_noise_device_* of path s.  The arrays hold the paths one behind the other: image and out of path s at s*W*H*3 elements,
 * features at s*W*H*8 elements, the state at byte s * rtw_temporal_state_bytes, the moment plane at byte s * rtw_history_moment_bytes, the
 * noise map at s*W*H elements.  The padding bytes between states and between moment planes (there whenever W*H is odd) are never written.
 * All paths of a call share t, c, n, the frame size and first-frame-ness: d_states_prev == NULL means every path resets.
 *   The table.  A device-resident step stays ONE launch with no hidden copy and no allocation (it can be captured into a graph like its
 * neighbours), so the per-path camera constants live in a caller-owned DEVICE table of 32 elements of T per path:
 *     0..2 origin, 3..5 lower_left_corner, 6..8 horizontal, 9..11 vertical of the path's CURRENT camera;
 *     12..14 origin, 15..17 w, 18..20 horizontal, 21..23 vertical of its PREVIOUS camera;
 *     24..28 Kw, Qh, Qv, ih, iv: with q = lower_left_corner - origin of the previous camera, q.w, q.horizontal, q.vertical,
 *     1 / horizontal.horizontal, 1 / vertical.vertical -- binary64 from the previous camera's fields, every dot product grouped
 *     (x + y) + z, each value rounded to T once (exactly what the single step derives from cam_prev);  29..31: 0.
 * rtw_reproject_table_* fills a HOST buffer of rtw_reproject_table_bytes bytes (pure host code; the caller uploads it); cams_prev == NULL
 * (first frames): elements 12..28 are 0.  A step whose d_states_prev is NULL reads no element of the table; any other reads 0..28.
 *   rtw_reproject_batch_device_*: one launch on `hip_stream`, asynchronous; rtw_stats() is left alone.  All pointers are DEVICE pointers.
 *   rtw_reproject_noise_batch_device_*: the n_paths maps of n_paths states and their moment planes, one launch.
 *   rtw_render_paths_*: n_paths paths of n_steps steps each in one call, host buffers, blocking, through the cached context.  The layout
 * is STEP-major, so that the frames of one step are contiguous: path s at step k is cams[k*n_paths + s], `seeds` holds n_steps*n_paths
 * values in the same order (or is NULL: p->seed), and frame (k, s) of `out` sits at (k*n_paths + s)*H*W*3.  On the context's stream:
 * ONE batched render of n_steps*n_paths views with gamma 0, ONE batched feature pass, ONE H2D of the whole table, n_steps batched step
 * launches (two sets of n_paths states -- with `n`, of moment planes -- ping-pong), with `n` one batched noise launch behind each step,
 * with `d` ONE plain or (with `n`) noise-guided batched filter pass over all frames, ONE D2H.  p->gamma is applied once, by the last stage
 * that runs.  `c`, `n`, `d`: the three combinations of rtw_render_path_clamped_* and additionally c == NULL (plain steps).  Path s equals,
 * on the bits, what rtw_render_sequence_*, rtw_render_path_guided_* or rtw_render_path_clamped_* returns for that path's cameras and
 * seeds.  rtw_stats() reports the render's record.
 *   Refusals, all decided before any HIP call: a null argument that is not optional -> -1; n_paths < 1, n_steps < 1 or a product
 * n_steps*n_paths beyond int32 -> -2; everything the single step, clamp and noise calls refuse, with that call's code; a table, feature
 * buffer, state or moment plane that is not 16-byte aligned, images, out or noise not aligned to T, outputs that alias each other or an
 * input over the full n_paths extents, exactly one of d_states_prev / d_moments_prev null when moments are on, `n` without `d`,
 * DEMODULATE flags of `t` and `d` that differ under `n` -> -2; width*height*frames >= 2^39 (the batched filter's rule) -> -5; the paths
 * call refuses everything the batched render, feature and filter calls refuse for n_steps*n_paths views, with that call's code.
 *   Left out on purpose: a host-buffer form of the single batched step (the paths call is the host form), paths of
 * different frame sizes or different t / c / n in one launch, a path that joins or resets alone mid-batch, device lists, the Julia shim,
 * one-call forms with the upsampler or the present stage behind them (the device-resident stages compose on the caller's stream).
 * Additive to ABI 4: detected by symbol lookup. */
int64_t rtw_reproject_table_bytes(int32_t n_paths, int32_t elem_bytes);
int rtw_reproject_table_f32(const rtw_camera_f32 *cams, const rtw_camera_f32 *cams_prev /* NULL: first frames */, int32_t n_paths, void *table /* host */);
int rtw_reproject_table_f64(const rtw_camera_f64 *cams, const rtw_camera_f64 *cams_prev /* NULL: first frames */, int32_t n_paths, void *table /* host */);
int rtw_reproject_batch_device_f32(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c /* may be NULL */, int32_t n_paths, const void *d_table, int32_t width,
                                   int32_t height, const void *d_images, const void *d_features, const void *d_states_prev /* NULL: first frames */,
                                   const void *d_moments_prev /* may be NULL */, void *d_states_next, void *d_moments_next /* may be NULL */, void *d_out,
                                   void *hip_stream);
int rtw_reproject_batch_device_f64(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c /* may be NULL */, int32_t n_paths, const void *d_table, int32_t width,
                                   int32_t height, const void *d_images, const void *d_features, const void *d_states_prev /* NULL: first frames */,
                                   const void *d_moments_prev /* may be NULL */, void *d_states_next, void *d_moments_next /* may be NULL */, void *d_out,
                                   void *hip_stream);
int rtw_reproject_noise_batch_device_f32(const rtw_temporal_noise_t *n, int32_t width, int32_t height, int32_t n_paths, const void *d_states, const void *d_moments,
                                         void *d_noise, void *hip_stream);
int rtw_reproject_noise_batch_device_f64(const rtw_temporal_noise_t *n, int32_t width, int32_t height, int32_t n_paths, const void *d_states, const void *d_moments,
                                         void *d_noise, void *hip_stream);
int rtw_render_paths_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_paths, int32_t n_steps, const uint64_t *seeds, const rtw_params *p,
                         const rtw_temporal_t *t, const rtw_temporal_clamp_t *c /* may be NULL */, const rtw_temporal_noise_t *n /* may be NULL */,
                         const rtw_denoise_t *d /* may be NULL */, float *out);
int rtw_render_paths_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_paths, int32_t n_steps, const uint64_t *seeds, const rtw_params *p,
                         const rtw_temporal_t *t, const rtw_temporal_clamp_t *c /* may be NULL */, const rtw_temporal_noise_t *n /* may be NULL */,
                         const rtw_denoise_t *d /* may be NULL */, double *out);

/* Temporal reuse over moving spheres: a first-hit motion pass and the step that reads it.  The steps above reproject a pixel's first-hit
 * point as if the world stood still; where a sphere moved between two frames they gather the history of the wrong place (a reset, or a
 * ghost).  One new pass says, per pixel, which sphere the pixel sees and how far that sphere moved since the previous frame; the step
 * subtracts that displacement from the world point before it projects.  Everything behind the projection -- taps, weights, blend, clamp,
 * moments, the noise map and the filters -- is what the blocks above define.
 * (The entry points are named rtw_motion_table_*, rtw_first_hit_motion_* and rtw_animated_step_*: the names of the blocks above are closed sets.)
 *
 * The definition.  Arithmetic is in T, every operation is rounded once, there is no FMA beyond what a numerics mode of hit(::Sphere)
 * itself contracts, quotients and sqrt are the correctly rounded IEEE ones.
 *   Motion plane.  H*W slots of 4 elements of T, each slot 16-byte aligned; pixel (i, j) at slot j*H + i holds (m.x, m.y, m.z, id):
 * m is the world-space displacement, since the previous frame, of the surface the pixel sees; id is the caller's index of the sphere
 * seen, as a value of T, or -1 for the sky.
 *   Motion table.  n slots of 4 elements in the caller's sphere order: (dx, dy, dz, 0).  rtw_motion_table_*(scene_prev, scene, table) is
 * pure host code like rtw_reproject_table_*: per component d = c_cur - c_prev, ONE subtraction in T; a sphere with k >= n_prev, or whose
 * radius differs bitwise from the previous scene's, is new or changed and gets three quiet NaNs, so that its pixels reset.  `table`
 * receives scene->n * 4 elements; the caller uploads it.
 *   The motion pass, per pixel.  The ray is the STEP's own ray, not a sample of the trace kernel: su, tv, D and nD exactly as in the
 * rtw_temporal_* block; origin = cam.origin, direction = nD, the lens is ignored.  Its first hit is what a scan of all n spheres finds
 * with hit(::Sphere) in the evaluation order of the numerics mode p->flags selects (RTW_FLAG_NUMERICS_*), tmin = 1e-4, tmax = +inf: the
 * smallest root t wins, and among equal roots the LOWER caller's index.  (The trace kernel's scans keep the reference's loop, in which the
 * later of two equal roots wins; the roots, and so the surface, are the same.)  A hit of sphere k gives the slot (table[k].xyz, T(k)); a miss
 * gives (0, 0, 0, -1); with a NULL table m = 0 and the pass is an id (picking) buffer.
 *   The motion step.  The plain step (rtw_temporal_device_*, rtw_history_moments_device_*) or the clamped one (rtw_clamped_step_device_*)
 * with ONE change: for a `has` pixel  d = ((origin + z*nD) - m) - origin_prev  per component, in this order; a sky pixel is unchanged.
 * A non-finite m makes d NaN, inr fails and the pixel resets: there is no extra rule.  The slot's fourth element has no effect on the
 * step.  With m = 0 everywhere the step is the step of the blocks above on the bits (x - 0 == x).
 * (tests/motion_ref.py restates all of this on the CPU and the device agrees on the bits.)
 *
 * rtw_first_hit_motion_device_*: ONE launch, asynchronous on `hip_stream` of the scene's device; of `p` the frame (width, height), the
 * device and the numerics bits are read -- RTW_FLAG_SCAN_VALU and RTW_FLAG_GROUP_CULL are accepted and change nothing; spp, max_depth, seed
 * and the chunks are not looked at.  `d_table` (scene n * 4 elements, may be NULL) and `d_motion` (H*W*4 elements) are 16-byte aligned
 * DEVICE pointers that do not overlap.  rtw_stats() is left alone.
 *   rtw_first_hit_motion_*: the host-buffer form, blocking, through the cached per-device context like rtw_render_features_f32 (the scene
 * is uploaded, or reused when its bytes are the same); `table` may be NULL.  rtw_stats() is left alone.
 *   rtw_animated_step_device_*: one step over a moving scene, ONE launch.  `c` NULL: no clamp; d_moment_prev and d_moment_next both NULL:
 * no moments -- the pointer rule of rtw_clamped_step_device_*.  cam_prev, d_state_prev and d_motion are NULL together: the first frame,
 * which runs the first-frame instance of the blocks above.  d_motion is 16-byte aligned and aliases no output.
 *   rtw_animated_step_*: the host-buffer form, blocking, through the one host path of rtw_temporal_f32; `motion` as d_motion.
 *   rtw_render_animation_*: n_frames frames of a scene that changes from frame to frame in one blocking call -- rtw_render_sequence_* /
 * rtw_render_path_clamped_* with a scene per frame.  `scenes` and `cams` hold n_frames entries (the spheres of all scenes in one order:
 * rtw_motion_table_* pairs them by index), `seeds` n_frames seeds (NULL: p->seed for every frame).  Per frame, on one stream of the cached
 * per-device context: the scene's upload (skipped while its bytes are those of the frame before), the render of `p` with gamma 0, the
 * feature pass over all of its chunks, from frame 1 on the motion table against the frame before and the motion pass (of p->flags it gets
 * the scan-mode and numerics bits), then the step -- frame 0 is a first frame; `c` non-NULL: clamped steps; no moments.  With `d`, ONE
 * batched filter pass (rtw_filter_batch_*'s launches) over the accumulated frames and their features follows.  ONE D2H of n_frames frames
 * into `out`; p->gamma is applied once, by the last stage that runs.  Frame v equals, on the bits, the chain of the single calls
 * (rtw_render_*, rtw_render_features_*, rtw_motion_table_*, rtw_first_hit_motion_*, rtw_animated_step_*, rtw_filter_batch_*), and with
 * n_frames identical scenes the call is rtw_render_sequence_* / rtw_render_path_clamped_* (n NULL) with the same arguments.  rtw_stats()
 * reports the counters of all frames' renders summed and the times of the slowest.
 *   Refusals, all decided before any HIP call: a null argument that is not optional -> -1; everything the step of the blocks above refuses,
 * with its code; exactly one of d_motion / d_state_prev (motion / state_prev) null, a motion plane or a table that is not 16-byte aligned,
 * a plane that overlaps the table or an output, width or height < 1, device < -1, flag bits other than the scan-mode and numerics ones, both
 * numerics bits -> -2; a scene (handle) of the other precision, p->device that is not the handle's -> -4; the frame rule -> -5.
 * rtw_render_animation_*: n_frames < 1, a negative sphere count -> -2; a null array of a scene that has spheres -> -1; everything
 * rtw_render_sequence_* / rtw_render_path_clamped_* refuses for n_frames views, with its code.
 *   Left out on purpose: batched paths with motion (rtw_reproject_batch_device_* has no motion planes),
 * a time per ray (true in-frame motion blur: the rtw_velocity_blur_* block below blurs a finished frame along the motion plane instead),
 * guided-filter and upsampler one-call forms, accumulators, device lists, the Julia shim.
 * Additive to ABI 4: detected by symbol lookup. */
int rtw_motion_table_f32(const rtw_scene_f32 *scene_prev, const rtw_scene_f32 *scene, void *table /* host */);
int rtw_motion_table_f64(const rtw_scene_f64 *scene_prev, const rtw_scene_f64 *scene, void *table /* host */);
int rtw_first_hit_motion_device_f32(rtw_scene_handle scene, const rtw_camera_f32 *cam, const rtw_params *p, const void *d_table /* may be NULL */,
                                    void *d_motion, void *hip_stream);
int rtw_first_hit_motion_device_f64(rtw_scene_handle scene, const rtw_camera_f64 *cam, const rtw_params *p, const void *d_table /* may be NULL */,
                                    void *d_motion, void *hip_stream);
int rtw_first_hit_motion_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cam, const rtw_params *p, const float *table /* may be NULL */, float *motion);
int rtw_first_hit_motion_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cam, const rtw_params *p, const double *table /* may be NULL */, double *motion);
int rtw_animated_step_device_f32(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c /* NULL: no clamp */, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev,
                                 int32_t width, int32_t height, const void *d_image, const void *d_features, const void *d_motion, const void *d_state_prev,
                                 void *d_state_next, const void *d_moment_prev, void *d_moment_next /* both NULL: no moments */, void *d_out, void *hip_stream);
int rtw_animated_step_device_f64(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c /* NULL: no clamp */, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev,
                                 int32_t width, int32_t height, const void *d_image, const void *d_features, const void *d_motion, const void *d_state_prev,
                                 void *d_state_next, const void *d_moment_prev, void *d_moment_next /* both NULL: no moments */, void *d_out, void *hip_stream);
int rtw_animated_step_f32(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c /* NULL: no clamp */, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev,
                          int32_t width, int32_t height, const float *image, const float *features, const float *motion, const void *state_prev, void *state_next,
                          const void *moment_prev, void *moment_next /* both NULL: no moments */, float *out);
int rtw_animated_step_f64(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c /* NULL: no clamp */, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev,
                          int32_t width, int32_t height, const double *image, const double *features, const double *motion, const void *state_prev, void *state_next,
                          const void *moment_prev, void *moment_next /* both NULL: no moments */, double *out);
int rtw_render_animation_f32(const rtw_scene_f32 *scenes, const rtw_camera_f32 *cams, int32_t n_frames, const uint64_t *seeds /* may be NULL */, const rtw_params *p,
                             const rtw_temporal_t *t, const rtw_temporal_clamp_t *c /* may be NULL */, const rtw_denoise_t *d /* may be NULL */, float *out);
int rtw_render_animation_f64(const rtw_scene_f64 *scenes, const rtw_camera_f64 *cams, int32_t n_frames, const uint64_t *seeds /* may be NULL */, const rtw_params *p,
                             const rtw_temporal_t *t, const rtw_temporal_clamp_t *c /* may be NULL */, const rtw_denoise_t *d /* may be NULL */, double *out);

/* Motion blur: a velocity-guided gather on the motion plane.  The 1-spp animation path renders every moving sphere razor sharp, so it
 * strobes; the motion plane of the block above says how far every pixel's surface moved.  This stage blurs a finished LINEAR frame along
 * that motion: a deterministic form of McGuire et al. 2012, "A Reconstruction Filter for Plausible Motion Blur" -- tile max, neighbour
 * max, a gather along the neighbourhood's dominant velocity with soft depth and velocity-aware weights; no jitter.  It sits between the
 * last linear stage (the step or the filter) and the present stage; it reads no temporal state and writes none, and its output must never
 * be fed back into the history.
 *
 * The definition.  Everything is computed in T; every operation is rounded once, no FMA; quotients and sqrt are the correctly rounded IEEE
 * ones; three-term sums are grouped (x + y) + z; a tap that does not take part is dropped by a select.  Pixel (i, j) is slot p = j*H + i.
 * Inputs: a LINEAR image (H*W*3), the features (H*W*8), the motion plane (H*W*4), `cam`, `cam_prev` and rtw_velocity_blur_t; output: an image
 * (H*W*3) that aliases no input.  clamp01(x) = x > 0 ? (x < 1 ? x : 1) : +0.
 *   Prepare.  valid, cov, has and z exactly as in the rtw_temporal_* block; zc = has ? z : +inf.
 *   Previous position.  Exactly the motion step's, with its host constants: for a `has` pixel d = ((origin + z*nD) - m) - origin_prev, for a
 * sky pixel d = nD (camera rotation blurs the sky); then dw, front, lam, s, t, x, y as defined there.  moved = valid and front and x and y
 * both finite;  u = moved ? (T(j) - x, T(i) - y) : (0, 0).
 *   Half-extent.  h = u * T(shutter/2) (the host rounds the factor once);  l2 = h.x*h.x + h.y*h.y;  if l2 > 256: h = h * (T(16) / sqrt(l2))
 * (one quotient, two products) and l2 is recomputed from the scaled h;  l = sqrt(l2).  The BLUR PLANE holds, at slot p, (h.x, h.y, zc, l) --
 * 16 or 32 bytes; zc is NaN for a pixel that is not valid.
 *   Tile max.  Tile (a, b) covers rows 16a .. 16a+15 and columns 16b .. 16b+15, clipped to the frame; TH = ceil(H/16), TW = ceil(W/16); its
 * index is b*TH + a.  Its value is the (h.x, h.y, l) of its pixel with the greatest l; among equals the lowest slot p wins (the rule is
 * associative: any reduction tree gives the same answer).  The TILE PLANE holds (h.x, h.y, l, 0) at slot b*TH + a.
 *   Neighbour max.  Over the up to nine tiles around a tile that lie in the frame: the greatest l, ties to the lowest tile index.  The
 * NEIGHBOUR PLANE holds (vN.x, vN.y, lN, 0) at slot b*TH + a.
 *   Gather, per valid pixel X = (i, j) with colour c, in tile (i/16, j/16).  If not lN >= T(0.5): out = c.  Otherwise lX = max(l_X, T(0.5)),
 * w0 = 1/lX, wsum = w0, sum[k] = c[k]*w0, and for n = 0 .. taps-1 except the middle one, n = (taps-1)/2:
 *       tt = T(2(n+1) - (taps+1)) / T(taps+1)
 *       qj = rint(T(j) + vN.x*tt);  qi = rint(T(i) + vN.y*tt)         (ties to even)
 *       a tap outside the frame or on a pixel that is not valid is skipped
 *       dist = sqrt(T(qj-j)*T(qj-j) + T(qi-i)*T(qi-i));  lY = max(l_q, T(0.5));  ext = T(depth_extent)
 *       soft depth compare of zc_q against zc_X: equal (both +inf included): f = b = 1; both finite: f = clamp01(1 - (zc_q - zc_X)/ext),
 *           b = clamp01(1 - (zc_X - zc_q)/ext); exactly one infinite: the finite one is in front -- zc_q finite: f = 1, b = 0, else f = 0,
 *           b = 1 -- decided by selects, never by arithmetic on an infinity
 *       cone(dist, l) = clamp01(1 - dist/l);  cyl(dist, l) = 1 - (x*x)*(3 - 2*x) with x = clamp01((dist - T(0.95)*l) / (T(0.1)*l))
 *       a = (f*cone(dist, lY) + b*cone(dist, lX)) + (cyl(dist, lY)*cyl(dist, lX))*2
 *       wsum = wsum + a;  sum[k] = sum[k] + a*c_q[k]
 * out[k] = sum[k] / wsum.  Then sqrt per channel if gamma = 1 (the pass-through pixels too).  A pixel that is not valid is a quiet NaN in
 * all three channels.  (tests/motion_blur_ref.py restates all of this on the CPU, twice, and the device agrees on the bits.)
 *   Workspace.  Caller-owned, rtw_velocity_blur_work_bytes(width, height, elem_bytes) bytes (monotone in the size; < 0: an error code), 16-byte
 * aligned: the blur plane at byte 0, the tile plane at byte 4*W*H*sizeof(T), the neighbour plane TH*TW slots behind it.  The layout is
 * public, like the state's.
 *
 * rtw_velocity_blur_device_*: THREE launches (velocity and tile max: a workgroup per tile; neighbour max; gather), asynchronous on
 * `hip_stream` of the device b->device (-1: the current one); rtw_stats() is left alone.  d_features, d_motion and d_work are 16-byte
 * aligned, d_image and d_out aligned to T; d_out and d_work alias neither each other nor any input.
 *   rtw_velocity_blur_*: the host-buffer form, blocking, through the cached per-device context like rtw_animated_step_f32.
 *   rtw_render_blurred_*: rtw_render_animation_* with the blur behind its last linear stage -- the same launches with gamma 0 up
 * to and including the steps (with `d`: the filter pass), one motion plane per frame kept, then for every frame from 1 on the three
 * launches above on (frame v, its features, its motion plane, cams[v], cams[v-1]) with gamma = p->gamma (b->gamma and b->device are
 * replaced); frame 0 has no previous camera and passes through with p->gamma applied (one launch).  ONE D2H as before.  Frame v equals, on
 * the bits, rtw_render_animation_* with p->gamma = 0 followed by rtw_velocity_blur_* on frame v.
 *   Refusals, all decided before any HIP call: a null argument -> -1; taps even or outside 3..31, unknown flags, gamma other than 0 or 1,
 * reserved != 0, device < -1, shutter outside (0, 1] or not finite, depth_extent not finite and positive, width or height < 1, elem_bytes
 * other than 4 or 8, misaligned or aliasing pointers -> -2; the denoiser's frame rule -> -5; the animation call additionally everything
 * rtw_render_animation_* refuses, with its code.
 *   Left out on purpose: batched views, upsampler and present one-call forms (the device stages compose on the
 * caller's stream), device lists, the Julia shim, jittered taps, lens-aware velocities, a time per ray.
 * Additive to ABI 4: detected by symbol lookup. */
#define RTW_VELOCITY_BLUR_TILE 16    /* the tile's edge and the largest half-extent of a blur, in pixels */
typedef struct {
    int32_t taps;               /* odd, 3..31: taps along the dominant velocity, the centre one is the pixel itself (default 15) */
    int32_t flags;              /* 0 */
    int32_t gamma;              /* 1 = sqrt per channel at the very end, 0 = linear */
    int32_t device;             /* -1 = current */
    int32_t reserved[2];        /* 0 */
    double  shutter;            /* in (0, 1]: the fraction of the frame interval the shutter is open, centred on the frame's time */
    double  depth_extent;       /* > 0, finite, world units: the softness of the depth compare (default 0.5) */
} rtw_velocity_blur_t;            /* 40 bytes */
int64_t rtw_velocity_blur_work_bytes(int32_t width, int32_t height, int32_t elem_bytes);
int rtw_velocity_blur_device_f32(const rtw_velocity_blur_t *b, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width, int32_t height,
                               const void *d_image, const void *d_features, const void *d_motion, void *d_work, void *d_out, void *hip_stream);
int rtw_velocity_blur_device_f64(const rtw_velocity_blur_t *b, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width, int32_t height,
                               const void *d_image, const void *d_features, const void *d_motion, void *d_work, void *d_out, void *hip_stream);
int rtw_velocity_blur_f32(const rtw_velocity_blur_t *b, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width, int32_t height,
                        const float *image, const float *features, const float *motion, float *out);
int rtw_velocity_blur_f64(const rtw_velocity_blur_t *b, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width, int32_t height,
                        const double *image, const double *features, const double *motion, double *out);
int rtw_render_blurred_f32(const rtw_scene_f32 *scenes, const rtw_camera_f32 *cams, int32_t n_frames, const uint64_t *seeds /* may be NULL */, const rtw_params *p,
                                     const rtw_temporal_t *t, const rtw_temporal_clamp_t *c /* may be NULL */, const rtw_denoise_t *d /* may be NULL */,
                                     const rtw_velocity_blur_t *b, float *out);
int rtw_render_blurred_f64(const rtw_scene_f64 *scenes, const rtw_camera_f64 *cams, int32_t n_frames, const uint64_t *seeds /* may be NULL */, const rtw_params *p,
                                     const rtw_temporal_t *t, const rtw_temporal_clamp_t *c /* may be NULL */, const rtw_denoise_t *d /* may be NULL */,
                                     const rtw_velocity_blur_t *b, double *out);

/* Depth of field: a gather on a finished pinhole frame.  Every stage behind the trace kernel takes its guides from the centre ray of a
 * pinhole camera; with a real aperture a low-sample frame is noisy exactly where it is out of focus, and there the guides no longer describe
 * the picture.  So: render through the pinhole, filter and accumulate on that frame, and apply the lens afterwards as a gather on the
 * finished LINEAR frame, driven by the depth the feature pass already wrote.  The stage is the sibling of the rtw_velocity_blur_* block: the
 * same place in the chain (behind the last linear stage, in front of the present stage), a caller-owned workspace with a public layout; its
 * guide is the feature buffer's depth plane.  The focus plane and the aperture become parameters of a cheap pass.
 *
 * The definition.  Everything is computed in T; every operation is rounded once, no FMA; quotients and sqrt are the correctly rounded IEEE
 * ones; three-term sums are grouped (x + y) + z; a tap that does not take part is dropped by a select.  Pixel (i, j) is slot p = j*H + i.
 * Inputs: a LINEAR image (H*W*3), the features (H*W*8), `cam` and rtw_defocus_t; output: an image (H*W*3) that aliases no input.
 * clamp01(x) = x > 0 ? (x < 1 ? x : 1) : +0;  min(a, b) = a < b ? a : b;  max(a, b) = a > b ? a : b  (in this argument order: a NaN on the
 * left gives b).
 *   Host constants, in binary64 over the camera's fields converted to binary64, each operation rounded once, then rounded once to T:
 * focus = ((o - llc).w) (per component o - llc, the dot product grouped as above), or focus_dist when that is > 0;  F = T(focus);
 * K = T((lens_radius * W) / sqrt(hor.hor)), the radius in pixels of the circle of confusion of a point at infinity;  Rm = T(max_radius).
 * The camera's own lens_radius is not read.  K is measured on the camera's OWN focus plane and does not move with focus_dist: an override f'
 * with lens radius r equals a camera rebuilt with its focus plane at f' (horizontal and vertical scaled by f'/f) and lens radius r*f'/f.
 *   Prepare.  valid, cov, has, z, su, tv, D and nD exactly as in the rtw_temporal_* block.  ca = -((nD.x*w.x + nD.y*w.y) + nD.z*w.z) with the
 * camera's w;  zax = z*ca, the depth along the optical axis.  A `has` pixel with zax > 0:  R = min(K * (|zax - F| / zax), Rm) -- one
 * difference, one abs, one quotient, one product, one min.  Every other valid pixel (sky; a surface at or behind the eye plane):
 * R = min(K, Rm).  zc = has ? z : +inf.  Rh = max(R, T(0.5));  w = 1 / (Rh*Rh).  The COC PLANE holds (R, zc, w, 0) at slot p -- 16 or 32
 * bytes; a pixel that is not valid holds (-1, NaN, 0, 0).
 *   Tile max.  Tile (a, b) covers rows 16a .. 16a+15 and columns 16b .. 16b+15, clipped to the frame; TH = ceil(H/16), TW = ceil(W/16); its
 * index is b*TH + a (the tiles of the rtw_velocity_blur_* block).  The TILE PLANE holds ONE element per tile: the greatest R of the tile's
 * pixels, -1 if none is valid.  A plain maximum: any reduction tree gives the same answer.
 *   Gather, per valid pixel X = (i, j) with colour c.  RN = the maximum of the tile plane over the up to nine tiles around X's tile that lie in
 * the frame.  If not RN >= T(0.5): out = c.  Otherwise m = ceil(RN + T(0.5)) - 1 as an integer (at most max_radius), wsum = +0,
 * sum = (+0, +0, +0), and for dj = -m .. m (outer, ascending), di = -m .. m (inner, ascending), the centre included, the tap q = (i+di, j+dj):
 *       a tap outside the frame or on a pixel that is not valid is skipped
 *       dist = sqrt(T(di*di + dj*dj))
 *       back = zc_q > zc_X                         (a comparison only: no arithmetic is done on an infinity)
 *       Rh_q = max(R_q, T(0.5));  Rh_X = max(R_X, T(0.5))
 *       lim = back and Rh_X < Rh_q                 (a tap BEHIND X never spreads further than X's own circle: background does not bleed
 *                                                   over sharp foreground)
 *       Re = lim ? Rh_X : Rh_q;  we = lim ? w_X : w_q
 *       cover = clamp01((Re + T(0.5)) - dist);  a tap with cover not > 0 is skipped
 *       a = cover*we;  wsum = wsum + a;  sum[k] = sum[k] + a*c_q[k]
 * out[k] = sum[k] / wsum (the centre tap always has cover = 1, so wsum > 0).  Then sqrt per channel if gamma = 1 (the pass-through pixels
 * too).  A pixel that is not valid is a quiet NaN in all three channels.  (tests/defocus_ref.py restates all of this on the CPU, twice, and
 * the device agrees on the bits.)
 *   Workspace.  Caller-owned, rtw_defocus_work_bytes(width, height, elem_bytes) bytes (monotone in the size; < 0: an error code), 16-byte
 * aligned: the CoC plane at byte 0, the tile plane at byte 4*W*H*sizeof(T), TH*TW elements rounded up to a multiple of four.  The layout
 * is public, like the state's.
 *
 * rtw_defocus_device_*: TWO launches (prepare and tile max: a workgroup per tile; the gather: a workgroup per tile over a window staged once
 * in LDS), asynchronous on `hip_stream` of the device b->device (-1: the current one); rtw_stats() is left alone.  d_features and d_work
 * are 16-byte aligned, d_image and d_out aligned to T; d_out and d_work alias neither each other nor any input.
 *   rtw_defocus_*: the host-buffer form, blocking, through the cached per-device context like rtw_velocity_blur_f32.
 *   rtw_render_defocused_*: the scene, the camera AS THE USER BUILT IT (with its aperture), the render's params, an optional filter and the
 * defocus: the render and the feature pass over all effective chunks run through a copy of the camera with lens_radius = 0, the filter (if
 * `d` is not NULL) follows, all with gamma 0; then the two launches above with gamma = p->gamma (b->gamma and b->device are replaced by
 * p's); ONE D2H.  Here and only here b->lens_radius == -1 means "the camera's own".  The result equals, on the bits, the chain of the
 * single calls on the pinhole copy -- rtw_render_* (or rtw_render_denoised_*) with gamma 0 and rtw_render_features_* -- followed by
 * rtw_defocus_*.  rtw_stats() afterwards reports the render's record.
 *   Refusals, all decided before any HIP call: a null argument -> -1 (`d` may be NULL); max_radius outside 1..8, unknown flags, gamma other
 * than 0 or 1, reserved != 0, device < -1, a lens_radius that is negative or not finite, a focus_dist that is negative or not finite, a
 * camera whose hor.hor or whose focus in use is not finite and positive, width or height < 1, elem_bytes other than 4 or 8, misaligned or
 * aliasing pointers -> -2; the denoiser's frame rule -> -5; the one-call form additionally everything rtw_render_features_* (and, with `d`,
 * rtw_denoise_*) refuses for its arguments, with its code.
 *   Left out on purpose: sequence, animation, upsampler and present one-call forms (the device stages compose on the
 * caller's stream); device lists; the Julia shim; radii beyond 8 px (a half-resolution pass); bokeh shapes; jittered taps.  (No longer left
 * out: batched views -- rtw_lens_batch_* below with max_radius <= 8.)
 * Additive to ABI 4: detected by symbol lookup. */
#define RTW_DEFOCUS_MAX_RADIUS 8     /* the largest circle of confusion, in pixels */
#define RTW_DEFOCUS_TILE 16          /* the tile's edge, in pixels */
typedef struct {
    int32_t max_radius;         /* 1..8: where the circle of confusion is clamped, in pixels (default 8) */
    int32_t flags;              /* 0 */
    int32_t gamma;              /* 1 = sqrt per channel at the very end, 0 = linear */
    int32_t device;             /* -1 = current */
    int32_t reserved[2];        /* 0 */
    double  lens_radius;        /* >= 0, finite, world units: half the aperture (rtw_render_defocused_* only: -1 = the camera's own) */
    double  focus_dist;         /* 0 = the camera's own focus plane; > 0, finite: an override */
} rtw_defocus_t;                /* 40 bytes */
int64_t rtw_defocus_work_bytes(int32_t width, int32_t height, int32_t elem_bytes);
int rtw_defocus_device_f32(const rtw_defocus_t *b, const rtw_camera_f32 *cam, int32_t width, int32_t height, const void *d_image, const void *d_features,
                           void *d_work, void *d_out, void *hip_stream);
int rtw_defocus_device_f64(const rtw_defocus_t *b, const rtw_camera_f64 *cam, int32_t width, int32_t height, const void *d_image, const void *d_features,
                           void *d_work, void *d_out, void *hip_stream);
int rtw_defocus_f32(const rtw_defocus_t *b, const rtw_camera_f32 *cam, int32_t width, int32_t height, const float *image, const float *features, float *out);
int rtw_defocus_f64(const rtw_defocus_t *b, const rtw_camera_f64 *cam, int32_t width, int32_t height, const double *image, const double *features, double *out);
int rtw_render_defocused_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cam, const rtw_params *p, const rtw_denoise_t *d /* may be NULL */,
                             const rtw_defocus_t *b, float *out);
int rtw_render_defocused_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cam, const rtw_params *p, const rtw_denoise_t *d /* may be NULL */,
                             const rtw_defocus_t *b, double *out);

/* Wide aperture: circles of confusion up to 32 px.  The block above clamps every circle of confusion at 8 px, and at the headline frame
 * size the headline camera sits at that clamp: lookfrom (13, 2, 3), vfov 20, focus 10, aperture 0.1 at 1920 x 1080 has K = 15.3 px.  This
 * stage is the standard remedy beside it: the frame is reduced by s = 2 or 4, the reduced copy is gathered by the SAME gather (a radius of
 * 32 px is 8 small pixels), and the result is blended back by the radius, so that what is nearly sharp keeps the full-resolution gather.
 * The existing entry points do not move: they keep refusing max_radius > 8.
 *
 * The definition, with the conventions of the block above: everything in T, every operation rounded once, no FMA, the correctly rounded
 * IEEE quotients and sqrt, what does not take part dropped by a select; clamp01, min and max as above.  Inputs and output are those of the
 * block above; rtw_wide_aperture_t has the fields of its struct with max_radius in 1..32.
 *   1. Scale.  s = 1 for max_radius <= 8: the call IS the one of the block above on the bits -- the same launches, the same workspace --
 * and nothing below applies.  s = 2 for 9..16, s = 4 for 17..32.  The small frame is h = ceil(H/s) rows by w = ceil(W/s) columns; small
 * pixel (a, b) is slot b*h + a.
 *   2. The narrow frame N: exactly the output of the block above with max_radius = 8 and gamma = 0 on the same inputs (its CoC plane and
 * tile plane are left in the head of the workspace).
 *   3. The wide CoC plane: Prepare and Tile max of the block above with Rm = T(max_radius).  A pixel with R < 8 carries the same R in both
 * planes on the bits.
 *   4. Reduce.  Small pixel (a, b) covers rows s*a .. s*a+s-1 and columns s*b .. s*b+s-1, clipped to the frame, visited with the column
 * outer and the row inner, both ascending.  Over the block's VALID pixels (their colour c from the input image, R and zc from the wide
 * plane), n of them:  csum[k] = csum[k] + c[k] and Rsum = Rsum + R, both from +0 in that order;  zmin = zc < zmin ? zc : zmin from +inf (a
 * comparison only; +inf stays when every valid pixel is sky);  c_s[k] = csum[k] / T(n);  R_s = (Rsum / T(n)) * T(1/s);  zc_s = zmin;
 * Rh_s = max(R_s, T(0.5));  w_s = 1 / (Rh_s*Rh_s).  The SMALL COLOUR holds c_s (3 elements per small pixel), the SMALL COC PLANE holds
 * (R_s, zc_s, w_s, 0).  A block with no valid pixel is not valid: its slot is (-1, NaN, 0, 0) and its colour (+0, +0, +0).  The SMALL TILE
 * PLANE holds the greatest R_s per 16 x 16 small tile (-1 if none is valid), index b'*th + a' with th = ceil(h/16): a plain maximum.
 * The sums are of at most 16 values, each <= Rm, and every k*Rm is a small integer: by monotone rounding every partial sum is <= k*Rm, the
 * mean is <= Rm and R_s <= Rm/s <= 8, so the window of the small gather is never exceeded.
 *   5. The small gather: Gather of the block above on the small frame -- the small colour as the image, the small CoC and tile planes --
 * with gamma = 0; every m there is at most ceil(max_radius / s).  Its output is the small image O (NaN where the small pixel is not valid).
 *   6. Compose, per valid pixel X = (i, j).  Rows: u = 2i + 1 - s;  a0 = floor(u / 2s) (floor division: -1 for the first rows);
 * fy = T(u - 2s*a0) / T(2s), an odd multiple of 1/2s, exact;  the taps are the small rows clamp(a0, 0, h-1) with weight 1 - fy and
 * clamp(a0+1, 0, h-1) with weight fy (both may be the same row).  Columns the same with v = 2j + 1 - s, b0, fx, w.  The four tap weights
 * are the products row weight * column weight (exact), visited in the order (row tap 0, column tap 0), (1, 0), (0, 1), (1, 1).  A tap on
 * a small pixel that is not valid is skipped;  ws = ws + wt,  acc[k] = acc[k] + wt*O_q[k], from +0;  U[k] = acc[k] / ws.  X's own block
 * holds X, so it is valid, and it is always one of the taps, with a positive weight: ws > 0.
 *       t = clamp01((R_X - T(4)) * T(0.25))        (R_X from the wide plane)
 *       out[k] = t <= 0 ? N[k] : (t >= 1 ? U[k] : N[k] + t*(U[k] - N[k]))
 * Then sqrt per channel if gamma = 1.  A pixel that is not valid is a quiet NaN in all three channels.  (tests/wide_aperture_ref.py
 * restates all of this on the CPU, twice, and the device agrees on the bits.)  A pixel with R < 4 is the narrow stage's on the bits; sharp
 * foreground in front of a wide background stays as sharp as the block above leaves it.
 *   Workspace.  Caller-owned, rtw_wide_aperture_work_bytes(width, height, elem_bytes, max_radius) bytes (monotone in the frame size; < 0:
 * an error code; for max_radius <= 8 what the block above reports), 16-byte aligned.  With r4(n) = n rounded up to a multiple of four,
 * t = TH*TW and t' = th*tw, the regions follow each other in this order, each beginning on a multiple of four ELEMENTS:
 *       the narrow stage's workspace    4*W*H + r4(t)      its CoC plane (Rm = 8) and tile plane
 *       the wide CoC plane              4*W*H
 *       the wide tile plane             r4(t)
 *       N                               r4(3*W*H)
 *       the small colour                r4(3*w*h)
 *       the small CoC plane             4*w*h
 *       the small tile plane            r4(t')
 *       O                               r4(3*w*h)
 * The layout is public, like the state's.
 *
 * rtw_wide_aperture_device_*: SIX launches for max_radius > 8 (prepare and gather of the block above with max_radius 8; prepare with
 * Rm = max_radius; reduce; the gather on the small frame; compose), TWO otherwise, asynchronous on `hip_stream` of the device b->device
 * (-1: the current one); rtw_stats() is left alone.  Alignment and aliasing as in the block above.
 *   rtw_wide_aperture_*: the host-buffer form, blocking, through the cached per-device context.
 *   rtw_render_wide_aperture_*: the one-call form of the block above with this stage at its end, argument for argument; here and only
 * here b->lens_radius == -1 means "the camera's own".  On the bits the chain of the single calls on the pinhole copy followed by
 * rtw_wide_aperture_*.
 *   Refusals, all decided before any HIP call: those of the block above with the same codes, max_radius outside 1..32 in place of 1..8;
 * rtw_wide_aperture_work_bytes refuses such a max_radius with -2 as well.
 *   Left out on purpose: sequence, animation, upsampler and present one-call forms; device lists;
 * the Julia shim (batched views no longer: rtw_lens_batch_* below); bokeh shapes; jittered taps; skipping the narrow gather on tiles that lie wholly at t >= 1 (no bit would change, but the
 * gather kernel would).  Additive to ABI 4: detected by symbol lookup. */
#define RTW_WIDE_APERTURE_MAX_RADIUS 32     /* the largest circle of confusion, in pixels */
typedef struct {
    int32_t max_radius;         /* 1..32: where the circle of confusion is clamped, in pixels; <= 8: the defocus stage itself */
    int32_t flags;              /* 0 */
    int32_t gamma;              /* 1 = sqrt per channel at the very end, 0 = linear */
    int32_t device;             /* -1 = current */
    int32_t reserved[2];        /* 0 */
    double  lens_radius;        /* >= 0, finite, world units: half the aperture (rtw_render_wide_aperture_* only: -1 = the camera's own) */
    double  focus_dist;         /* 0 = the camera's own focus plane; > 0, finite: an override */
} rtw_wide_aperture_t;          /* 40 bytes */
int64_t rtw_wide_aperture_work_bytes(int32_t width, int32_t height, int32_t elem_bytes, int32_t max_radius);
int rtw_wide_aperture_device_f32(const rtw_wide_aperture_t *b, const rtw_camera_f32 *cam, int32_t width, int32_t height, const void *d_image,
                                 const void *d_features, void *d_work, void *d_out, void *hip_stream);
int rtw_wide_aperture_device_f64(const rtw_wide_aperture_t *b, const rtw_camera_f64 *cam, int32_t width, int32_t height, const void *d_image,
                                 const void *d_features, void *d_work, void *d_out, void *hip_stream);
int rtw_wide_aperture_f32(const rtw_wide_aperture_t *b, const rtw_camera_f32 *cam, int32_t width, int32_t height, const float *image, const float *features,
                          float *out);
int rtw_wide_aperture_f64(const rtw_wide_aperture_t *b, const rtw_camera_f64 *cam, int32_t width, int32_t height, const double *image, const double *features,
                          double *out);
int rtw_render_wide_aperture_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cam, const rtw_params *p, const rtw_denoise_t *d /* may be NULL */,
                                 const rtw_wide_aperture_t *b, float *out);
int rtw_render_wide_aperture_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cam, const rtw_params *p, const rtw_denoise_t *d /* may be NULL */,
                                 const rtw_wide_aperture_t *b, double *out);

/* Batched lens stages: N views, or ONE frame under N lens settings, in each launch.  A stereo pair, a grid of previews or N candidate
 * cameras go through one batched render, one batched feature pass and one batched filter; the block above then costs N x 6 launches.  And
 * the first thing a user does with a lens that is a parameter of a cheap pass is a focus pull or an aperture bracket: one rendered frame
 * under N lenses.  Both are the batch below: n_views views in the SIX launches of the block above (TWO for max_radius <= 8, where the batch
 * is the batched defocus stage -- there is one family of names, rtw_lens_*, for both stages), whatever n_views is.  There is no new
 * arithmetic.
 *
 * The definition.  View v of the batch is, bit for bit, rtw_wide_aperture_device_* with cams[v], lens_radii[v], focus_dists[v] and b's
 * max_radius and gamma on frame v: the image and every region of the workspace.
 *   The lens table.  rtw_lens_table_* (pure host code) writes 32 elements of T per view into the HOST buffer `table`
 * (rtw_lens_table_bytes(n_views, elem_bytes) = 32*n_views*elem_bytes bytes); the caller uploads it.  Elements 0..28 are the entry
 * rtw_reproject_table_* writes for cams[v] as its own previous camera; element 29 is F = T(focus) and element 30 is
 * K = T((lens_radius*W) / sqrt(hor.hor)) -- the host constants of the rtw_defocus_* block, computed in binary64 and rounded to T once, with
 * focus = focus_dists[v] if > 0, else the camera's own; element 31 is 0.  lens_radii NULL: b->lens_radius for every view; focus_dists NULL:
 * b->focus_dist for every view.  Every view passes the checks of the single stage; the first offending view is named in rtw_last_error.
 *   Layout.  Views follow each other in the arrays: the output of view v at v*W*H*3 elements; the workspace of view v at byte
 * v * rtw_wide_aperture_work_bytes(W, H, elem_bytes, max_radius), with the single stage's public layout inside (that size is a multiple of
 * 16 bytes); rtw_lens_batch_work_bytes is n_views times the single value.  n_frames is n_views -- image and features of view v
 * at v*W*H*3 and v*W*H*8 elements -- or 1: every view reads frame 0, the focus or aperture bracket.  Outputs and workspaces are per view
 * either way.
 *
 * rtw_lens_batch_device_*: SIX launches for max_radius > 8, TWO otherwise, asynchronous on `hip_stream` of the device b->device;
 * no hidden copy, no allocation; rtw_stats() is left alone.  Of `b` only max_radius, gamma, device, flags and reserved are read: the
 * per-view lens lives in the DEVICE table d_table.  d_table, d_features and d_work are 16-byte aligned, d_images and d_out aligned to T.
 *   rtw_lens_batch_*: the host-buffer form, blocking, through the cached per-device context: one H2D per input and of the table
 * (built inside), the launches, ONE D2H.
 *   rtw_render_lens_batch_*: ONE batched render of the pinhole copies with gamma 0, ONE batched feature pass over all effective
 * chunks, with `d` ONE batched filter pass, ONE H2D of the table, the batched stage with gamma = p->gamma (b's gamma and device replaced
 * by p's), ONE D2H.  Here and only here a lens_radii[v] -- or b->lens_radius when the array is NULL -- of -1 means "cams[v]'s own".  View
 * v equals, on the bits, rtw_render_wide_aperture_* with cams[v] and p->seed = seeds[v] (seeds NULL: p->seed).  rtw_stats() reports the
 * render's record.
 *   Refusals, all decided before any HIP call: a null argument that is not optional -> -1; n_views < 1, n_frames other than 1 or n_views,
 * everything the single stage refuses (with its code), a table, feature buffer or workspace that is not 16-byte aligned, images or out
 * not aligned to T, outputs that alias each other or an input over the FULL batch extents (inputs counted once when n_frames == 1), a
 * lens_radii or focus_dists entry the single stage would refuse -> -2; width*height*n_views >= 2^39 (the batched filter's rule) -> -5; the
 * one-call form additionally everything rtw_render_features_batch_* and rtw_filter_batch_* refuse for its arguments, with their codes.
 *   Left out on purpose: views of different sizes or different max_radius / gamma in one launch; a batched motion
 * blur (no batched motion pass exists to feed it); sequence, animation, upsampler and present one-call forms; device lists; the Julia shim.
 * Additive to ABI 4: detected by symbol lookup. */
int64_t rtw_lens_table_bytes(int32_t n_views, int32_t elem_bytes);
int rtw_lens_table_f32(const rtw_wide_aperture_t *b, const rtw_camera_f32 *cams, int32_t n_views, int32_t width, int32_t height,
                       const double *lens_radii /* may be NULL */, const double *focus_dists /* may be NULL */, void *table);
int rtw_lens_table_f64(const rtw_wide_aperture_t *b, const rtw_camera_f64 *cams, int32_t n_views, int32_t width, int32_t height,
                       const double *lens_radii /* may be NULL */, const double *focus_dists /* may be NULL */, void *table);
int64_t rtw_lens_batch_work_bytes(int32_t width, int32_t height, int32_t elem_bytes, int32_t max_radius, int32_t n_views);
int rtw_lens_batch_device_f32(const rtw_wide_aperture_t *b, int32_t n_views, int32_t n_frames, const void *d_table, int32_t width, int32_t height,
                                       const void *d_images, const void *d_features, void *d_work, void *d_out, void *hip_stream);
int rtw_lens_batch_device_f64(const rtw_wide_aperture_t *b, int32_t n_views, int32_t n_frames, const void *d_table, int32_t width, int32_t height,
                                       const void *d_images, const void *d_features, void *d_work, void *d_out, void *hip_stream);
int rtw_lens_batch_f32(const rtw_wide_aperture_t *b, const rtw_camera_f32 *cams, int32_t n_views, int32_t n_frames, const double *lens_radii /* may be NULL */,
                                const double *focus_dists /* may be NULL */, int32_t width, int32_t height, const float *images, const float *features, float *out);
int rtw_lens_batch_f64(const rtw_wide_aperture_t *b, const rtw_camera_f64 *cams, int32_t n_views, int32_t n_frames, const double *lens_radii /* may be NULL */,
                                const double *focus_dists /* may be NULL */, int32_t width, int32_t height, const double *images, const double *features, double *out);
int rtw_render_lens_batch_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds /* may be NULL */, const rtw_params *p,
                                       const rtw_denoise_t *d /* may be NULL */, const rtw_wide_aperture_t *b, const double *lens_radii /* may be NULL */,
                                       const double *focus_dists /* may be NULL */, float *out);
int rtw_render_lens_batch_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds /* may be NULL */, const rtw_params *p,
                                       const rtw_denoise_t *d /* may be NULL */, const rtw_wide_aperture_t *b, const double *lens_radii /* may be NULL */,
                                       const double *focus_dists /* may be NULL */, double *out);

/* Present stage: display-ready 8-bit frames from the device.  Every pipeline above ends in T elements in the column-major layout of the
 * render entry points; a window, a PNG or a video encoder wants 8-bit rows.  One kernel clips, rounds, packs and transposes in HBM, and the
 * D2H behind it moves 3 or 4 bytes per pixel instead of 12 or 24.
 *
 * The definition.  Input: a frame of H*W*3 elements of T in the layout of the render entry points, pixel (i, j) (0-based row, column) at
 * (j*H + i)*3; a batch is n_views such frames one behind the other.  Output: H*W*C bytes, ROW-major: channel k of pixel (i, j) at
 * (i*W + j)*C + k, C = channels (3 or 4); rows are tightly packed, row 0 is the row a PNG or PPM writer writes first; a batch is n_views
 * frames of H*W*C bytes one behind the other, and rtw_present_bytes returns the total (n_views == 0 means one frame; < 0: an error code).
 *   Per channel k < 3, on the input element x, every operation in binary64 and rounded once (no FMA), whatever T is:
 *     1. v = (double)x                                  (exact for both T)
 *     2. if v is NaN the byte is nan_rgb[k] and steps 3 - 7 are skipped   (decided per channel, not per pixel)
 *     3. v = v * exposure
 *     4. v = min(max(v, 0), 1)                          (+inf gives 1; -inf and -0.0 give 0)
 *     5. with RTW_PRESENT_SQRT: v = sqrt(v), the correctly rounded IEEE one   (the reference's gamma 2, for linear inputs such as a temporal state)
 *     6. y = v * 255.0
 *     7. without RTW_PRESENT_DITHER: the byte is q = rint(y), ties to even
 *        with RTW_PRESENT_DITHER:    q = min(floor(y + t), 255),  t = (B(i mod 8, j mod 8) + 0.5) / 64   (exact in binary64)
 *           B(r, c) = sum over b = 0..2 of  (((r^c)>>b)&1) << (5-2b)  |  ((r>>b)&1) << (4-2b)
 *        the standard 8 x 8 Bayer index matrix (its first row is 0 32 8 40 2 34 10 42); the same t serves all three channels of a pixel
 *        and every view of a batch.
 *   With RTW_PRESENT_BGR channels 0 and 2 of the output are swapped; that applies to nan_rgb too, which is given in R, G, B order.  With
 * C = 4 byte 3 is 255.
 *   With exposure = 1, no flags and nan_rgb = {0, 0, 0} the output is imageio.to_u8 -- rint(clip(x, 0, 1) * 255) in binary64, NaN -> 0, the
 * 8-bit image the project already defines -- of the same frame on the bits.  (tests/present_ref.py restates the definition on the CPU and
 * the device agrees on the bytes.)
 *
 * rtw_present_device_* / rtw_present_batch_device_*: ONE launch, asynchronous on `hip_stream` (a hipStream_t as void*; NULL = the null stream)
 * of the device p->device (-1: the current one).  `d_image` is aligned to T, `d_out` to 4 bytes; the output may not overlap the input.
 * Neither changes what rtw_stats() reports.
 *   rtw_present_*: the host-buffer form of one frame, blocking, on the per-device stream and buffer cache of rtw_render_f32: the frame in,
 * the kernel, one D2H of the bytes.
 *   rtw_render_presented_* / rtw_render_presented_batch_*: render and present in one call on the cached context's stream.  `d` NULL: the
 * render of rtw_render_f32 / rtw_render_batch_f32 with p->gamma as given (whole frames on one device: what a feature render of `params`
 * refuses is refused).  `d` non-NULL: exactly what rtw_render_denoised_* / rtw_render_filtered_batch_* do, up to their device image.  Then
 * the present kernel (p->device replaced by params->device) and ONE D2H of rtw_present_bytes bytes: no float frame crosses the bus.
 * rtw_stats() reports the render as it does after those calls; view v of the batch equals the single call on the bits.
 *   Refusals, all decided before any HIP call: a null argument -> -1 (`d` may be NULL); channels other than 3 or 4, unknown flag bits,
 * reserved != 0, an exposure that is not finite and positive, width or height < 1, n_views < 1 on a batch call (< 0 for rtw_present_bytes),
 * device < -1, a d_out that is not 4-byte aligned, a d_image that is not aligned to T, an output that overlaps the input -> -2; 2^31 tiles
 * of 64 x 64 pixels or more over all views (what the launch's index arithmetic covers) -> -5; the render-and-present calls additionally
 * refuse everything their render (and, with `d`, their filter) refuses.
 *   Left out on purpose: the sRGB transfer curve (its pow is not correctly rounded, so a device and a numpy witness
 * could not be held to the same bits), a row pitch, a vertical flip, 16-bit output, one-call forms for the accumulator, the upsampler and
 * the sequences (their device-resident stages compose with rtw_present_device_*), a host-buffer batch form.
 * Additive to ABI 4: detected by symbol lookup. */
#define RTW_PRESENT_DITHER 1       /* ordered dither (8 x 8 Bayer) instead of round-to-nearest */
#define RTW_PRESENT_BGR 2          /* bytes in B, G, R order */
#define RTW_PRESENT_SQRT 4         /* sqrt per channel after the clamp: gamma 2 for a linear input */
typedef struct {
    int32_t channels;           /* 3 or 4: bytes per pixel (byte 3 = 255) */
    int32_t flags;              /* RTW_PRESENT_* */
    int32_t device;             /* -1 = current */
    uint8_t nan_rgb[3];         /* the bytes of a NaN channel, in R, G, B order */
    uint8_t reserved0;          /* 0 */
    double  exposure;           /* > 0, finite: multiplies every channel before the clamp */
    int32_t reserved[2];        /* 0 */
} rtw_present_t;                /* 32 bytes */
int64_t rtw_present_bytes(int32_t width, int32_t height, int32_t channels, int32_t n_views);
int rtw_present_device_f32(const rtw_present_t *p, int32_t width, int32_t height, const void *d_image, void *d_out, void *hip_stream);
int rtw_present_device_f64(const rtw_present_t *p, int32_t width, int32_t height, const void *d_image, void *d_out, void *hip_stream);
int rtw_present_batch_device_f32(const rtw_present_t *p, int32_t width, int32_t height, int32_t n_views, const void *d_images, void *d_out,
                                 void *hip_stream);
int rtw_present_batch_device_f64(const rtw_present_t *p, int32_t width, int32_t height, int32_t n_views, const void *d_images, void *d_out,
                                 void *hip_stream);
int rtw_present_f32(const rtw_present_t *p, int32_t width, int32_t height, const float *image, uint8_t *out);
int rtw_present_f64(const rtw_present_t *p, int32_t width, int32_t height, const double *image, uint8_t *out);
int rtw_render_presented_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cam, const rtw_params *params, const rtw_denoise_t *d /* may be NULL */,
                             const rtw_present_t *p, uint8_t *out);
int rtw_render_presented_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cam, const rtw_params *params, const rtw_denoise_t *d /* may be NULL */,
                             const rtw_present_t *p, uint8_t *out);
int rtw_render_presented_batch_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds,
                                   const rtw_params *params, const rtw_denoise_t *d /* may be NULL */, const rtw_present_t *p, uint8_t *out);
int rtw_render_presented_batch_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds,
                                   const rtw_params *params, const rtw_denoise_t *d /* may be NULL */, const rtw_present_t *p, uint8_t *out);

/* Ray queries: the closest hit of caller-supplied rays against the whole sphere list.  Everything above reaches the intersection routine
 * through pixels; this block hands it out as it is -- for picking under a position that is no pixel centre, visibility and shadow tests
 * between points, collision and line-of-sight queries, light baking, or an integrator of the caller's own on the host.
 *
 * The definition.  Arithmetic is in T; nothing is normalised.
 *   A ray is 8 elements of T, rays one behind the other: ox, oy, oz, dx, dy, dz, tmax, tag.  `tag` is the caller's (a pixel index, a
 * payload) and is never read.  Directions are expected to be of unit length to rounding, as every ray of the reference is (its hit()
 * drops `a`); the result is nevertheless DEFINED for every finite ray as what the formula gives, without a normalisation.  tmax = +inf
 * is legal; other non-finite elements are outside the contract.
 *   The result for ray i is idx[i] (int32_t) and, where asked for, 8 elements of T at rec[8 i]: t, px, py, pz, nx, ny, nz, front.
 * idx[i] is the sphere's 0-based index in the CALLER's list, or -1; front is 1 or 0; the record is all +0 on a miss.
 *   The values are those of the reference's hit(::HittableList) with (tmin, tmax_i), in the numerics mode of the call's flags
 * (RTW_FLAG_NUMERICS_*), on the bits: the spheres are tested in the caller's order, `closest` starts at tmax_i, a root is rejected when
 * root < tmin || closest < root -- so the LATER of two spheres with the same root wins (the reference's rule, not the motion pass's) --
 * and the record is p = o + t d, n_out = (p - c) / r, front = d.n_out < 0, n = front ? n_out : -n_out, each operation rounded once.
 * tmin is one value per call; tmax lives in the ray.
 *
 * rtw_rays_params.  flags: RTW_FLAG_SCAN_VALU and the two RTW_FLAG_NUMERICS_* bits (they exclude each other); RTW_FLAG_GROUP_CULL is
 * accepted and runs the same scans, as the feature pass does; any other bit -> -2.  device: as in rtw_params.  max_workgroups: 0 =
 * automatic, otherwise >= 1, a cap on the kernel's persistent grid -- scheduling only, the words are identical for every value.
 * reserved: 0.  tmin: finite and >= 0, converted to T once; 1e-4 is the reference's.
 *
 * rtw_cast_rays_device_*: ONE launch, asynchronous on `hip_stream` of the scene's device, re-entrant like rtw_render_features_device_*.
 * `d_rays` (n * 8 elements) and `d_rec` (n * 8 elements, may be NULL: indices only) are 16-byte aligned DEVICE pointers, `d_idx` (n
 * int32_t) is 4-byte aligned; nothing beyond ray n - 1 is read or written.  rtw_stats() afterwards reports samples = segments = n,
 * sphere_tests = n x spheres and the kernel time.
 *   rtw_cast_rays_*: the host-buffer form, blocking, through the cached per-device context like rtw_render_features_f32 (the scene is
 * uploaded, or reused when its bytes are the same): one H2D of the rays, one launch, one D2H of `idx` and, where asked for, one of `rec`.
 *   Refusals, all decided before any HIP call: a null argument other than rec -> -1; n < 0, a flag bit that is not named above, both
 * numerics bits, reserved != 0, device < -1, max_workgroups < 0, a tmin that is not finite or is negative, d_rays or d_rec not 16-byte
 * aligned, d_idx not 4-byte aligned, host buffers that overlap -> -2; a handle of the other precision or of another device -> -4;
 * n >= 2^31 -> -5.  n == 0 -> 0 with nothing enqueued (rtw_stats() is left alone).
 *   Left out on purpose: an early-exit any-hit mode (rec == NULL is the occlusion query today, and it pays the full
 * scan), the group cull on caller rays, a tmin per ray, scatter and shading of the hits, device lists, the Julia shim.
 * Additive to ABI 4: detected by symbol lookup. */
typedef struct {
    int32_t flags;            /* RTW_FLAG_SCAN_VALU, RTW_FLAG_GROUP_CULL, RTW_FLAG_NUMERICS_*                    */
    int32_t device;           /* HIP ordinal, or -1 = the current device (device form: the handle's)         */
    int32_t max_workgroups;   /* 0 = automatic, else a cap on the persistent grid (scheduling only)          */
    int32_t reserved;         /* 0                                                                           */
    double tmin;              /* finite, >= 0; converted to T once (the reference's: 1e-4)                   */
} rtw_rays_params;            /* 24 bytes */
int rtw_cast_rays_device_f32(rtw_scene_handle scene, const void *d_rays, int64_t n, const rtw_rays_params *p, void *d_idx, void *d_rec /* may be NULL */,
                             void *hip_stream);
int rtw_cast_rays_device_f64(rtw_scene_handle scene, const void *d_rays, int64_t n, const rtw_rays_params *p, void *d_idx, void *d_rec /* may be NULL */,
                             void *hip_stream);
int rtw_cast_rays_f32(const rtw_scene_f32 *scene, const float *rays, int64_t n, const rtw_rays_params *p, int32_t *idx, float *rec /* may be NULL */);
int rtw_cast_rays_f64(const rtw_scene_f64 *scene, const double *rays, int64_t n, const rtw_rays_params *p, int32_t *idx, double *rec /* may be NULL */);

/* Radiance queries: ray_color along caller-supplied rays.  The ray queries above stop at the hit; this block runs the whole Monte Carlo
 * estimate the renders are built around -- scan, scatter, sky, bounce by bounce -- on rays that belong to no pixel and no camera: light
 * and irradiance probes, light baking at surface points, reflection captures, radiance along the rays of a caller's own camera model
 * (fisheye, orthographic, panoramas), the continuation of paths a caller started itself.
 *
 * The definition.  Arithmetic is in T, colour in binary64; nothing is normalised.
 *   The input is the ray list of the ray queries as it stands: n rays of 8 elements of T, ox oy oz dx dy dz tmax tag, so one buffer serves
 * both calls.  Elements 6 and 7 are not read: ray_color scans with tmin = T(1e-4) and tmax = +inf.
 *   Sample s in [0, spp) of ray i is the reference's ray_color(scene, o_i, d_i, max_depth) (src/ray_color.jl:14-38; the product of the
 * attenuations formed front to back, as every render here forms it) on a FRESH stream: the stream rule of the renders (DESIGN.md
 * section 5) with seed, p = first_stream + i in the place of the pixel and c = first_sample + s in the place of the chunk.  One stream
 * per SAMPLE, on purpose: the result does not depend on how samples are dealt to lanes, waves or launches.  No camera draw happens: the
 * first draw of a stream belongs to the first scatter.
 *   The result for ray i is three binary64 values at out[3 i]: the three channel sums of its spp radiances in 64.64 fixed point (the
 * pixel's exact sum), each rounded once to binary64 and divided by (double)spp.  They are linear -- no gamma, no conversion to T: a caller
 * weights and sums them further.  `out` is n x 3 binary64 in both precisions.
 *   Poisoning: a sample radiance that is NaN, infinite or >= 2^31 makes all three values of that ray NaN (the pixel's rule).
 *   Every finite ray has a defined result; non-finite rays are outside the contract.  Directions longer than 1.0009 and far origins take
 * the scan's slow path, unchanged.
 *   Two consequences.  A list traced in two calls, the second with first_stream advanced by the first call's n, gives the words of the
 * one call.  A ray placed twice in a list gets two independent estimates (and that is how one ray gets more lanes than one today).
 * Another seed, first_stream or first_sample moves the words of a ray whose path draws a direction and reaches the sky (a first hit on
 * a Lambertian sphere, say); it need not move a ray that misses at once (sky(d) on every stream), one that starts inside an opaque
 * sphere (black on every stream) or one that meets only glass and polished metal (a stream decides a choice there, not a direction).
 *
 * rtw_trace_params.  flags: RTW_FLAG_SCAN_VALU and the two RTW_FLAG_NUMERICS_* bits (they exclude each other); RTW_FLAG_GROUP_CULL is
 * accepted and runs the plain scans, as in the ray queries; any other bit -> -2.  device: as in rtw_params.  max_workgroups: 0 =
 * automatic, otherwise >= 1, a cap on the launch grid -- scheduling only, the words are identical for every value.  spp >= 1.  max_depth:
 * the range rtw_params.max_depth has, [0, 2^22) (0: every sample is black).  reserved: 0.  seed, first_stream, first_sample: above.
 *
 * The device form (suffix _device_f32 / _device_f64): ONE launch, asynchronous on `hip_stream` of the scene's device, re-entrant like the
 * device form of the ray queries.  `d_rays` (n * 8 elements) is a 16-byte aligned DEVICE pointer, `d_out` (n * 3 binary64) an 8-byte
 * aligned one; nothing beyond ray n - 1 is read or written.  rtw_stats() afterwards reports samples = n x spp, segments = the scans with
 * a live ray (the reference's count), sphere_tests = segments x spheres and the kernel time.
 *   The host-buffer form (suffix _f32 / _f64): blocking, through the cached per-device context like the host form of the ray queries: one
 * H2D of the rays, one launch, one D2H of `out`.
 *   Refusals, all decided before any HIP call: a null argument -> -1; n < 0, a flag bit that is not named above, both numerics bits,
 * reserved != 0, device < -1, max_workgroups < 0, spp < 1, max_depth outside its range, first_stream + n or first_sample + spp beyond
 * 2^64 - 1, d_rays not 16-byte aligned, d_out not 8-byte aligned, host buffers that overlap -> -2; a handle of the other precision or of
 * another device -> -4; n >= 2^31 -> -5.  n == 0 -> 0 with nothing enqueued (rtw_stats() is left alone).
 *   Left out on purpose: one ray's samples split across lanes (few rays x very many samples: repeat the ray in the
 * list, with first_sample apart), the group cull on caller rays, tmin or tmax per ray, the exact sums as an output (resumable passes),
 * device lists, the Julia shim.
 * Additive to ABI 4: detected by symbol lookup. */
typedef struct {
    int32_t flags;            /* RTW_FLAG_SCAN_VALU, RTW_FLAG_GROUP_CULL, RTW_FLAG_NUMERICS_*                    */
    int32_t device;           /* HIP ordinal, or -1 = the current device (device form: the handle's)         */
    int32_t max_workgroups;   /* 0 = automatic, else a cap on the launch grid (scheduling only)              */
    int32_t spp;              /* samples per ray, >= 1                                                       */
    int32_t max_depth;        /* ray_color's depth, [0, 2^22) (the reference's default: 16)                  */
    int32_t reserved;         /* 0                                                                           */
    uint64_t seed;            /* the stream seed                                                             */
    uint64_t first_stream;    /* stream index of ray 0: ray i draws from stream first_stream + i             */
    uint64_t first_sample;    /* index of the first sample: sample s is chunk first_sample + s of the stream */
} rtw_trace_params;           /* 48 bytes */
int rtw_trace_rays_device_f32(rtw_scene_handle scene, const void *d_rays, int64_t n, const rtw_trace_params *p, void *d_out, void *hip_stream);
int rtw_trace_rays_device_f64(rtw_scene_handle scene, const void *d_rays, int64_t n, const rtw_trace_params *p, void *d_out, void *hip_stream);
int rtw_trace_rays_f32(const rtw_scene_f32 *scene, const float *rays, int64_t n, const rtw_trace_params *p, double *out);
int rtw_trace_rays_f64(const rtw_scene_f64 *scene, const double *rays, int64_t n, const rtw_trace_params *p, double *out);

/* Counters/timings of the last render issued from this thread (waits for it to finish). */
int rtw_stats(rtw_stats_t *out);

/* The shards of the last render issued from this thread, one entry per shard in shard order (a device list of N: N entries; one
 * device: one): the HIP ordinal it ran on and the HIP-event time of its trace kernel.  *count receives the number of shards; at most
 * `capacity` entries are written.  (rtw_stats_t.kernel_ms is the maximum of these.) */
int rtw_stats_devices(int32_t capacity, int32_t *count, int32_t *devices, double *kernel_ms);

/* Unit-level device entry points used by the parity tests (tier T0): each evaluates the
 * device implementation of one reference function on `count` inputs, one lane per input.
 * All pointers are HOST pointers; layouts are documented in tests/test_gpu_units.py.
 *   op: 0 hit_sphere  1 reflect  2 refract  3 reflectance  4 scatter  5 get_ray  6 skycolor
 *       7 rng_f (uniforms from a stream state)  8 hit_world  9 ray_color
 *       10 hit_world, scene staged in LDS  11 hit_world_cull (RTW_FLAG_GROUP_CULL)
 *       12 exact 64.64 fixed-point accumulation of 8 doubles
 *       13 hit_world_mfma (pass 1 on the matrix pipe: the trace kernel's plain scan), scene staged in LDS;
 *          tmin of ray 0 serves the whole launch, tmax is +inf
 *       14 the same with block culling (RTW_FLAG_GROUP_CULL on the matrix pipe), cull layout staged in LDS
 *       15 near_zero(v) (src/vec.jl:19-20)
 *       16 (Float32) the kernels' short correctly-rounded sqrt / reciprocal against the compiler's IEEE sequences on a range of binary32 bit patterns:
 *          in = (first pattern, count) per item, out = (mismatches sqrt, mismatches 1/x, first bad pattern of each or -1)
 *       17 - 20 the scans of ops 10, 11, 13, 14 with a candidate sink: what pass 1 hands pass 2 (tests/test_gpu_filters.py)
 *   Ops 21 - 23 run the accumulator's tile kernels (the adaptive render's stopping rule, its tile lists, its per-tile resolve) on words
 *   the caller makes up, with the launch geometry of rtw_render_adaptive_*.  Their layouts belong to the whole call, not to an item, in
 *   8-byte slots: "value" slots hold a binary64 number (integers as such), "raw" slots a uint64 / int64.  Tiles are 8 x 8 pixels,
 *   n_tiles = ceil(height / 8) * ceil(width / 8), tile t = (j / 8) * ceil(height / 8) + i / 8 for row i, column j; the words of a frame
 *   are rtw_accum_read_pixels' (pixel (i, j) at (j * height + i) * 8).  Nulls -> -1; a size or value outside the layout, a frame of more
 *   than 16384 on a side or 2^20 pixels, or more than 2^24 input slots -> -2; all before any HIP call.  Ops 21 and 22 are on rtw_unit_f64 only.
 *       21 the tile check.  count = n_views >= 1.  in: 8 value slots width, height, c, chunk_spp, tolerance, dark_floor, 0, 0; then per
 *          view n_tiles value slots C_t and width * height * 8 raw words.  out (raw int64): per view the n_tiles flags of the single
 *          call's check kernel, launched view by view; then the n_views * n_tiles flags of ONE launch of the batch's check kernel.  A
 *          flag is 1 for a tile with C_t == c that is NOT converged under the rule with n = c * chunk_spp, 0 for every other tile.
 *       22 the tile lists.  count = n >= 1 flags.  in: n raw slots, the low 32 bits of each are the flag (set: non-zero).  out (raw
 *          int64): the count and the n list slots of the single call's one-workgroup compaction, then the same of the batch's count /
 *          scan / scatter.  A list holds the indices of the set flags in ascending order; the slots behind the count hold -1.
 *       23 the per-tile resolve (also on rtw_unit_f32: T = float).  count = 1.  in: 8 value slots width, height, spp, chunk_spp, gamma
 *          (0 / 1), 0, 0, 0; n_tiles value slots C_t >= 1; width * height * 8 raw words.  out: width * height * 3 value slots, element
 *          (j * height + i) * 3 + channel: the sum over min(spp, C_t * chunk_spp) samples of the pixel's tile, rounded to T, widened.
 *   Op 25 runs the noise map kernel of rtw_accum_noise_* the same way (24 is not an op; also on rtw_unit_f32: T = float).  count = 1.  in: 8 value
 *          slots width, height, spp, chunk_spp, dark_floor (finite, >= 0), 0, 0, 0; n_tiles value slots C_t >= 1; width * height * 8 raw words.
 *          out: width * height value slots, element j * height + i: the map's value of type T, widened (NaN for a poisoned pixel).
 *       26 one bounce as the trace kernel composes it (needs a scene; per item like ops 0 - 20).  in: state[2] (raw), o[3], d[3].  hit_world as op 8
 *          with tmin = 1e-4, tmax = +inf, then on the UPLOADED material rows the kernel's own sequence: make_hitrec, the dielectric constants
 *          1 / ir, r0_front, r0_back the upload stored, scatter_begin with them, attenuation_of, the rejection loop, scatter_finish, the final
 *          normalize.  out: state[2] (raw), idx, o[3], d[3], att[3]; a miss leaves the state as it came, idx = -1 and zeros.
 *       27 op 20's scan with a sink that also records the block vote of the group cull (needs a scene of at most 512 spheres with matrix-pipe
 *          cull operands; per item like ops 17 - 20).  in: o[3], d[3], tmin, tmax.  out: the 18 slots of op 20 -- ok, mf_sc, candidate bits
 *          [8 raw uint64], in-lane bits [8 raw uint64], bit i = sphere i of the caller's list -- and one raw uint64: bit b is set when block b
 *          of the cull layout's device order was voted for by the half wave of this ray (item i runs in lane i % 64 of wave i / 64; lanes
 *          behind `count` have no ray).  tests/test_gpu_cull_vote.py
 *       28 the cull layout (needs a scene with matrix-pipe cull operands).  Item p is device position p, its block is p / 32.  in: one slot,
 *          ignored.  out: the caller's index of the sphere at that position, or -1 for a dead or padding slot and for p beyond the layout;
 *          1 if the position is in the in-lane list (tested by every lane itself, its filter row disabled), else 0; the number of positions;
 *          the number of blocks.
 *   Ops 30 and 31 run the batched per-tile resolve and the batched noise map of rtw_accum_resolve_batch_* / rtw_accum_noise_batch_* the same
 *          way (29 is not an op, like 24; both also on rtw_unit_f32: T = float).  count = n_views >= 1.  in: the 8 header slots of op 23 (30:
 *          width, height, spp, chunk_spp, gamma, 0, 0, 0) or of op 25 (31: ..., dark_floor, 0, 0, 0); then per view n_tiles value slots C_t >= 1
 *          and width * height * 8 raw words.  With E = width * height * 3 (30) or width * height (31): out = per view the E value slots of the
 *          single kernel of op 23 / op 25, launched view by view; then the n_views * E value slots of ONE launch of the batch kernel, view v
 *          at v * E.  tests/test_gpu_accum_filter_batch.py
 *   Ops 32 - 35 are the candidate sinks 17 - 20 with a flush counter (scenes of at most 512 spheres; per item like ops 17 - 20: the scans of ops 10,
 *          11, 13, 14 in turn).  in: o[3], d[3], tmin, tmax.  out: the 18 slots of the sink and one raw uint64 of four 16-bit counts: how often a
 *          full candidate list was resolved early during this ray's scan -- bits 0-15 A (the block loop of the matrix-pipe scan), 16-31 B (its
 *          in-lane filter class, group cull), 32-47 C (the explode loop of its pass 2): ops 34 and 35; bits 48-63 D (the all-VALU scan, op 32)
 *          or E (the all-VALU cull scan, op 33: the lane's own count; A - D are the wave's, in every live row alike).  36 is the first number
 *          behind the last op.  tests/test_gpu_list_caps.py
 *   bits 8-9 of `op`: the numerics mode of the ray-sphere test for ops 0, 8 - 11, 13, 14, 17 - 20, 26, 27, 32 - 35 (0 reference, 1 contract, 3 reference_fma2; 2 is rejected)  */
int rtw_unit_f32(int op, int count, const void *in, void *out, const rtw_scene_f32 *scene,
                 const rtw_camera_f32 *cam);
int rtw_unit_f64(int op, int count, const void *in, void *out, const rtw_scene_f64 *scene,
                 const rtw_camera_f64 *cam);

/* Frees the cached per-device render records (counters, events).  Optional.  Afterwards
 * rtw_stats() reports "no render" on every thread until that thread renders again. */
int rtw_shutdown(void);

#ifdef __cplusplus
}
#endif
#endif
