// rtw_host.hpp -- host-side internals of librtw_hip.so shared by its translation units (nothing here is part of the C ABI):
//   rtw_abi.hip          the extern "C" entry points (include/rtw_hip.h) that no other unit defines, argument validation, the per-device contexts and the per-render
//                        records behind rtw_stats(): begin_record / run_record, the one sequence around every launch that has a record
//   rtw_scene.hip        scene upload: SoA rows, kd split of the group-cull layout, the f16-split operands of the matrix-pipe filter
//   rtw_launch.hip       one render = one launch of the trace kernel (rtw_kernels.hpp / rtw_pool.hpp): geometry, occupancy, job shape, views
//   rtw_render_host.hip  the host-buffer entry points that render: the pool of cached per-device contexts (scene, stream, buffer), ONE one-device path (render_one_device)
//                        behind render, batch, feature and the composite render + stage calls, the motion pass, the accumulator's filtered call, or a device list
//   rtw_stage_host.hip   the pure stages on host buffers (filter, present, upsampler, temporal step, motion blur, the lens stages): ONE path (stage_one_device) behind all of them
//                        (rtw_host_ctx.hpp: what the two share -- the lease of a context, that path and render_one_device on top of it, the regions of the device buffer;
//                        rtw_layout.hpp: the regions' byte arithmetic and the alias check, plain C++)
//   rtw_multi.hip        what a device list needs: peer access, the on-demand RCCL binding, the un-tile kernel
//   rtw_batch_accum_f32.hip / _f64.hip  the BATCH && ACCUM instances of the trace kernel (rtw_instances.hpp: the kernel-instance table), a unit per precision
//   rtw_features_accum_batch_f32.hip / _f64.hip  the TILED && BATCH instances of the feature kernel (rtw_features.hpp), a unit per precision
//   rtw_accum.hip        progressive and adaptive render: the accumulator object (rtw_accum.hpp), its passes, the adaptive loop, the read-only passes, export / import
//   rtw_accum_kernels.hip  the accumulator's kernels (merge, resolve, tile check / compaction, noise map; single and batched), their launches and the unit ops on them
//   rtw_unit.hip         the T0 unit entry points (rtw_units.hpp)
//   rtw_features.hip     first-hit feature buffers: one launch of the feature kernel (rtw_features.hpp) for one view or a batch of views, the device-resident entry points
//   rtw_rays.hip         ray queries: closest hits of caller-supplied rays -- their checks, one launch of the ray kernel (rtw_rays.hpp), the device-resident entry points
//   rtw_trace_rays.hip   radiance queries: ray_color of caller-supplied rays -- their checks, one launch of the radiance kernel (rtw_trace_rays.hpp), the device-resident entry points
//   rtw_denoise.hip      the feature-guided denoiser: its checks, the launch sequence of its kernels (rtw_denoise.hpp) for one frame or a batch of frames, the device-resident entry points
//   rtw_upsample.hip     the feature-guided upsampler: its checks, the launch sequence (the denoiser's prepare and level kernels at the small size, then rtw_upsample.hpp at the full size), the device-resident entry points
//   rtw_temporal.hip     temporal reprojection: its checks, the host constants and the one launch of a step for one path or a batch of paths (rtw_temporal.hpp; clamped: rtw_temporal_clamp.hpp), the device-resident entry points
//   rtw_motion.hip       the first-hit motion pass over moving spheres: its checks, the motion table, the one launch of its kernel (rtw_motion.hpp), the device-resident entry points
//   rtw_motion_blur.hip  the motion-blur stage on the motion plane: its checks, the workspace, the three launches of its kernels (rtw_motion_blur.hpp), the device-resident entry points
//   rtw_defocus.hip      the defocus stage (depth of field on the depth plane) and the lens family's checks of one view in their four parts, the host constants (one view's entry of the lens table), the two launches of its kernels (rtw_defocus.hpp) for one view or a batch of views
//   rtw_wide_aperture.hip  the wide-aperture stage (circles of confusion up to 32 px): the six launches (the defocus stage's kernels at two sizes, rtw_wide_aperture.hpp between and behind them) for one view or a batch of views, the checks of N views, the lens table, ONE device-resident entry point (lens_device) behind the defocus, wide-aperture and batched ones
//   rtw_present.hip      the present stage: its checks, the one launch of its kernel (rtw_present.hpp) for one frame or a batch, the device-resident entry points
//   (rtw_scene_view.hpp: what both launch functions derive from their arguments; rtw_instances.hpp: the one table of the trace kernel's instances)
// A function that exists once per precision and crosses units is declared here ONCE, as a template under its own name, and the unit that
// defines it ends with its two explicit instantiations (float with rtw_camera_f32 / rtw_scene_f32, double with the _f64 structs); a caller
// names the precision it has -- launch_temporal<T>(...) -- and the struct types are deduced.  Declared in this form:
//   rtw_scene.hip upload_scene; rtw_launch.hip launch_render, upload_views; rtw_features.hip launch_features; rtw_rays.hip launch_rays; rtw_trace_rays.hip launch_trace_rays; rtw_denoise.hip launch_denoise;
//   rtw_upsample.hip launch_upsample; rtw_temporal.hip launch_temporal, temporal_table, launch_temporal_noise; rtw_motion.hip launch_motion,
//   motion_table; rtw_motion_blur.hip launch_motion_blur; rtw_defocus.hip validate_lens, launch_defocus, launch_defocus_prepare,
//   launch_defocus_gather, lens_table_entry; rtw_wide_aperture.hip launch_wide_aperture, validate_lens_batch, lens_table; rtw_present.hip
//   launch_present; rtw_unit.hip run_unit; rtw_accum.hip validate_ / enqueue_accum_features and their _batch forms (on the camera alone).
// Not in this form: batch_accum_kernel_f32 / _f64 and features_tiled_batch_kernel_f32 / _f64, each half in a unit of its own so that the heavy
// trace instances compile in parallel.  StageMarks (below) is the one measurement aid of the stages' launch functions.
// Everything is in namespace rtwh with hidden visibility; the library exports the C ABI only.
#pragma once
#pragma GCC visibility push(default)
#include "../../include/rtw_hip.h"
#pragma GCC visibility pop

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#pragma GCC visibility push(hidden)

#include "rtw_layout.hpp"

namespace rtw { struct DevCounters; }      // rtw_kernels.hpp (device side); the host keeps one per render record


// ---- device scene handle (the C ABI's opaque rtw_scene_handle) ------------------------------------
struct rtw_scene_dev {
    int device;
    int is_f64;
    int n, n_pad;
    void *geom, *mat0, *mat1;
    void *scan;      // Float64: the binary32 filter array of pass 1 (8 floats per sphere); Float32: null (geom itself)
    // pass 1 on the matrix pipe (hit_world_mfma): A operands per block of 32 spheres, scales and the ray's share of the margin
    void *mf_ops;    // null: the scene's extent is outside what the f16 split covers (the VALU scan is used)
    int mf_blocks;
    float mf_sc, mf_sigma2, mf_oo_keep, mf_o1_coef, mf_o_max, mf_mr;
    int n_huge, huge[2];   // spheres that pass the filter for nearly every ray (a ground sphere): tested exactly by every lane, their filter rows disabled
    // the plain matrix-pipe scan of the trace kernel runs over its OWN order (rtw_plain_layout.hpp: spatially sorted, evenly filled blocks; the
    // huge spheres behind the blocks): operands, geom / mat0 / mat1 rows and the caller's index of every row.  Set whenever mf_ops is.
    // (p_alias: the caller's order is kept -- at most one block, or the A/B aid -- and geom / mat0 / mat1 / mf_ops are the arrays above)
    void *p_mf_ops, *p_geom, *p_mat0, *p_mat1;
    unsigned short *p_orig;
    int p_alias, p_n, p_n_pad, p_mf_blocks, p_huge[2];
    // group-cull mode on the matrix pipe: the same operands in the cluster-major order + one box per block of 32
    void *c_mf_ops, *c_mf_box;
    float c_glo[3], c_ghi[3];   // the box of the whole small class (union of the block boxes): the ray is clipped against it once per scan
    int c_mf_blocks;
    float c_grid[6];       // the bins of the per-ray block vote (rtw::CullGrid: inv[3], off[3]); its tables lie behind the boxes in c_mf_box
    int c_n_inlane, c_inlane[8];   // spheres of the cluster-major order that every lane tests by itself (rtw::RTW_CULL_INLANE_MAX): the huge spheres and, when it fits, the whole BIG class
    // opt-in group-cull mode (RTW_FLAG_GROUP_CULL): cluster-major copies
    void *c_bound, *c_exact, *c_mat0, *c_mat1;
    unsigned short *c_orig;
    int c_groups_pad, c_big;
    double c_cs[3], c_rs;
    uint64_t content_hash;   // FNV-1a over the precision tag, n and the nine host arrays at upload: what binds a progressive accumulator to its scene
};

namespace rtwh {

extern __thread char g_err[512];         // (__thread: no dynamic initialisation, so no init-function call through a hidden weak symbol from the other translation units)
int fail(int code, const char *fmt, ...);

// Measurement / test switches of the environment are honoured only under the master switch RTW_ENABLE_TEST_AIDS=1 (read once):
// without it a stray RTW_SCAN=valu or RTW_JOB_PIXELS=1 in a caller's environment changes nothing (include/rtw_hip.h).
bool test_aids();
const char *aid_env(const char *name);
bool aid_flag(const char *name);

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return ::rtwh::fail((int)e_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// for calls whose failure cannot be acted upon (frees on cleanup paths): RTW_DEBUG=1 reports them on stderr
#define HIP_IGNORE(expr)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            static const bool dbg_ = ::rtwh::aid_env("RTW_DEBUG") != nullptr;                          \
            if (dbg_) fprintf(stderr, "[rtw debug] %s -> %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            (void)hipGetLastError();            /* do not leave it for a later hipGetLastError() check */ \
        }                                                                                     \
    } while (0)

// The measurement aid of the stages (tools/gpu_*.py; RTW_DENOISE_PROFILE, RTW_TEMPORAL_PROFILE, RTW_PRESENT_PROFILE, each read once per
// process by the launch function that owns the `static const bool` it hands in): events around every launch of a stage.  Off -- the
// production path -- mark() does nothing and no event is ever created, recorded or destroyed.  On: mark() puts an event on the stream
// (one in front of the first launch, one behind every launch; at most MAX: the upsampler's `levels` + 3), measure() blocks until the last
// one has happened and fills ms[k], the time between marks k and k + 1, and total_ms, from the first mark to the last; the launch function
// prints them.  The events are destroyed on every return path.
struct StageMarks {
    static constexpr int MAX = 11;
    const bool on;
    const hipStream_t stream;
    hipEvent_t e[MAX] = {};
    int n = 0;
    float ms[MAX - 1] = {}, total_ms = 0;
    StageMarks(bool on_, hipStream_t stream_) : on(on_), stream(stream_) {}
    StageMarks(const StageMarks &) = delete;
    ~StageMarks() { for (int k = 0; k < n; ++k) HIP_IGNORE(hipEventDestroy(e[k])); }
    hipError_t mark() {
        if (!on) return hipSuccess;
        if (n == MAX) return hipErrorInvalidValue;
        if (hipError_t rc = hipEventCreate(&e[n])) return rc;
        return hipEventRecord(e[n++], stream);          // (counted before it is recorded: the destructor destroys it either way)
    }
    hipError_t measure() {
        if (n < 2) return hipErrorInvalidValue;
        if (hipError_t rc = hipEventSynchronize(e[n - 1])) return rc;
        for (int k = 0; k + 1 < n; ++k) if (hipError_t rc = hipEventElapsedTime(&ms[k], e[k], e[k + 1])) return rc;
        return hipEventElapsedTime(&total_ms, e[0], e[n - 1]);
    }
};

// restores the caller's current device when an entry point returns
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceGuard() { if (prev >= 0) HIP_IGNORE(hipSetDevice(prev)); }
};

// ---- per-render record: device counters + the events that time the trace kernel ---------------
struct RenderRec {
    int device = -1;
    rtw::DevCounters *ctr = nullptr;     // device memory
    rtw::DevCounters *h_ctr = nullptr;   // pinned host copy: filled by an asynchronous D2H behind the kernel on the render's stream (no blocking copy per render)
    size_t ctr_bytes = 0;                // how much of it that copy brought over (the head; everything with the drain profile)
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;      // around the kernel; behind the copy of the counters
    bool used = false;                   // ev1 has been recorded at least once
    bool done = true;                    // the kernel recorded by ev1 is known to have finished (no hipEventQuery needed)
    bool owned = false;                  // referenced by some thread's "last render"
    bool fresh = true;                   // the device counters have never been cleared as a whole
    int n_spheres = 0, n_chunks = 0, grid = 0, block = 256;
    void *d_views = nullptr, *h_views = nullptr;  // batched renders: the views' cameras + seeds (device copy; pinned staging for its H2D)
    size_t views_cap = 0;
    ~RenderRec() {
        if (ctr) HIP_IGNORE(hipFree(ctr));
        if (h_ctr) HIP_IGNORE(hipHostFree(h_ctr));
        if (d_views) HIP_IGNORE(hipFree(d_views));
        if (h_views) HIP_IGNORE(hipHostFree(h_views));
        if (ev2) HIP_IGNORE(hipEventDestroy(ev2));
        if (ev0) HIP_IGNORE(hipEventDestroy(ev0));
        if (ev1) HIP_IGNORE(hipEventDestroy(ev1));
    }
};

// ---- persistent context of the host-buffer entry points (rtw_render_f32/_f64) -----------------------
// What a caller that renders frame after frame through the Julia `render()` shim pays per call, besides the kernel, is the
// image D2H: the uploaded scene (kd split + matrix-pipe operands: a dozen hipMalloc + synchronous copies), the stream and the
// device image are kept per device and reused while the scene's bytes are the same.
struct HostCtx {
    int device = -1;
    bool busy = false;                       // in use by a render call (guarded by DeviceCtx::mu)
    hipStream_t stream = nullptr;
    rtw_scene_handle scene = nullptr;        // the cached upload ...
    std::vector<unsigned char> scene_key;    // ... and the exact bytes it was made from (precision tag, n, the nine arrays)
    void *d_img = nullptr;  size_t d_cap = 0;      // device image / compact shard
    void *d_aux = nullptr;  size_t aux_cap = 0;    // multi-device root: the gathered compact shards
    hipEvent_t done_ev = nullptr;                  // multi-device: this shard has arrived in the root's gather buffer
    void *h_stage = nullptr; size_t stage_cap = 0; // multi-device without peer access: pinned staging of this shard
    unsigned long long last_use = 0;               // pool eviction: least recently used idle entry
    ~HostCtx();
};

struct DeviceCtx {
    int device = -1;
    int num_cus = 0;
    size_t lds_per_cu = 0;                         // hipDeviceProp_t::maxSharedMemoryPerMultiProcessor (160 KB on MI355X)
    std::vector<std::pair<std::pair<const void *, size_t>, int>> occupancy;   // (kernel, dynamic LDS) -> workgroups per CU (asked of the runtime once; guarded by mu)
    std::mutex mu;
    std::vector<std::unique_ptr<RenderRec>> recs;
    std::vector<std::unique_ptr<HostCtx>> host;    // at most RTW_HOST_CTX_POOL cached entries
    std::map<int, bool> peer;                      // peer device -> access enabled in both directions (ensure_peer)
    unsigned long long use_clock = 0;
};
#define RTW_HOST_CTX_POOL 8          // cached host contexts per device at most (what concurrent callers can hold)
#define RTW_HOST_CTX_IDLE_KEEP 3     // ... of which idle ones kept for other scenes (acquire_host)
using CtxPtr = std::shared_ptr<DeviceCtx>;       // holders keep a context alive across a concurrent rtw_shutdown()


extern std::atomic<unsigned> g_generation;      // bumped by rtw_shutdown: invalidates every thread's "last render"

void release_last();
// what rtw_stats() reports: the records of the last render issued from this thread
struct LastRender {
    unsigned generation = 0;
    bool resolved = false;
    std::vector<RenderRec *> recs;          // pending (device-resident call) or already summed into `agg`
    std::vector<CtxPtr> ctxs;               // the contexts that own `recs` (kept alive; parallel to recs)
    rtw_stats_t agg;
    std::vector<std::pair<int, double>> per_device;   // (device ordinal, kernel ms) of every shard of the last render, in shard order (rtw_stats_devices)
    ~LastRender();                          // a thread that exits hands its records back
};
extern thread_local LastRender g_last;
void hold_last(RenderRec *rec, const CtxPtr &ctx);       // the record of a device-resident call (null: none) stays with this thread for rtw_stats()

int get_ctx(int device, CtxPtr *out);
int acquire_rec(DeviceCtx *ctx, RenderRec **out);           // a record nobody references whose previous kernel (if any) has finished; the device must be current
void release_rec(const CtxPtr &ctx, RenderRec *r, bool finished);
// The sequence around every launch that has a record.  begin_record: a record (acquire_rec) that describes the launch, the first `ctr_bytes`
// of its counters -- what comes back to the host -- cleared on `stream`; *rec_out is set as soon as a record exists, so the caller can hold
// it after a late error.  run_record: ev0, `launch()` (it enqueues the kernel and nothing else), ev1, the counters' copy, ev2.
int begin_record(DeviceCtx *ctx, const rtw_scene_dev *scene, int n_chunks, int grid, int block, size_t ctr_bytes, hipStream_t stream, RenderRec **rec_out);
template <typename Launch>
int run_record(RenderRec *rec, hipStream_t stream, Launch launch) {
    HIP_TRY(hipEventRecord(rec->ev0, stream));
    (void)hipGetLastError();           // (hipEventQuery's hipErrorNotReady in acquire_rec must not be mistaken for a launch failure)
    launch();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(rec->ev1, stream));
    HIP_TRY(hipMemcpyAsync(rec->h_ctr, rec->ctr, rec->ctr_bytes, hipMemcpyDeviceToHost, stream));     // (into pinned memory: truly asynchronous)
    HIP_TRY(hipEventRecord(rec->ev2, stream));
    rec->used = true; rec->done = false;
    return 0;
}
int resolve_device(int device, int *out);
int validate_params(const rtw_params *p, int *n_chunks, int *chunk_spp);
int check_chunk_range(int32_t begin, int32_t count, int nch);     // [begin, begin + count) lies inside a render's `nch` effective chunks
long long local_tiles(const rtw_params *p);

template <typename SceneT> bool s_has_bad_scene(const SceneT *s) {
    return s->n > 0 && (!s->cx || !s->cy || !s->cz || !s->r || !s->kind || !s->ar || !s->ag || !s->ab || !s->param);
}

// the element type of a camera struct (rtw_camera_f32 / _f64), for a caller that is a template on the camera alone (rtw_accum.hip)
template <typename CamT> using CamElem = std::remove_extent_t<decltype(CamT::origin)>;

struct SceneDeleter { void operator()(rtw_scene_dev *h) const { rtw_scene_free(h); } };
using ScenePtr = std::unique_ptr<rtw_scene_dev, SceneDeleter>;

// rtw_scene.hip
template <typename T, typename SceneT> int upload_scene(const SceneT *s, int device, rtw_scene_handle *out);

// rtw_launch.hip -- enqueue one render (this shard's tiles) on `stream`; `rec` receives the counters and the kernel's events.
// n_views == 0: one render of the camera `cams` points to.  n_views >= 1: a batch of that many views (validate_batch first): `cams` /
// `seeds` (null: p->seed) hold n_views entries, `d_out` n_views frames.
// `pass`: one pass of a progressive render (rtw_accum.hip has validated it): the chunks [chunk_begin, chunk_begin + chunk_count) of the render
// `p` describes are added to `words` (layout: include/rtw_hip.h rtw_accum_read_pixels); `samples` = the samples the accumulator holds
// after this pass, the divisor of the running image written to `d_out` (null: none).  `adapt`: a pass of an adaptive render (the ADAPT
// kernels: half differences in word 7); `tile_list` non-null: only the `list_tiles` tiles of that device-resident list
// A pass of a BATCH of such renders (n_views >= 1): `views` holds every view's accumulator and divisor (`words` / `samples` of the
// pass itself are unused), `tile_list` numbers the tiles batch-globally, v * n_tiles + t
struct AccumViewPass { unsigned long long *words; int samples; };
struct AccumPass { unsigned long long *words; int chunk_begin, chunk_count, samples; bool adapt = false; const int *tile_list = nullptr; int list_tiles = 0; const AccumViewPass *views = nullptr; };
template <typename T, typename CamT>
int launch_render(rtw_scene_handle scene, const CamT *cams, int n_views, const uint64_t *seeds, const rtw_params *p, void *d_out, hipStream_t stream, RenderRec **rec_out, CtxPtr *ctx_out, const AccumPass *pass = nullptr);
// a batch's cameras and seeds (null: `seed` for every view) into the record's pinned buffer and, by ONE asynchronous H2D on `stream`, into its
// device buffer (the upload of launch_render's batches): *d_cams receives the device array of n_views rtw::Camera<T>, *d_seeds that of the seeds.
// `tiles` non-null: n_views device pointers (the tile-chunk arrays of adaptive accumulators) travel behind them, *d_tiles receives the table's device address
template <typename T, typename CamT>
int upload_views(RenderRec *rec, const CamT *cams, int n_views, const uint64_t *seeds, uint64_t seed, hipStream_t stream, const void **d_cams, const unsigned long long **d_seeds,
                 const int *const *tiles = nullptr, const int *const **d_tiles = nullptr);
int resolve_rec(RenderRec *r, rtw_stats_t *agg);            // wait for a record's kernel and add its counters to `agg`
// what the kernel-instance table answers (rtw_instances.hpp): the kernel, and whether it has the default numerics mode compiled in
struct TraceInstance { const void *kern; bool fixed; };
// rtw_batch_accum_f32.hip / _f64.hip: the BATCH && ACCUM (&& ADAPT) instance of the trace kernel for a scan variant, as launch_render chooses
// among the other instances (`fixed`: the numerics mode is the default one, which the headline variants have compiled in)
TraceInstance batch_accum_kernel_f32(bool cull, bool mfma, bool lds_scene, bool fixed, bool adapt);
TraceInstance batch_accum_kernel_f64(bool cull, bool mfma, bool lds_scene, bool fixed, bool adapt);
// rtw_abi.hip: the checks of a batched render that need no device (include/rtw_hip.h rtw_render_batch_f32)
int validate_batch(const void *cams, int32_t n_views, const rtw_params *p, const void *out);
// Below the C ABI n_views == 0 is the single-view call and n_views >= 1 a batch of that many.  A batched entry point hands its caller's count
// down through batch_views: a count that is no batch stays one the batch's validation refuses (-2) and never selects the single-view path.
inline int32_t batch_views(int32_t n_views) { return n_views < 1 ? -1 : n_views; }
// The alias check of an entry point (rtw_layout.hpp first_alias: the outputs against each other, then against the inputs; absent ranges
// skipped): the first offending pair is refused with -2.  `input_word`: what an input is called where the call has exactly one.
inline int check_alias(std::initializer_list<ByteRange> outs, std::initializer_list<ByteRange> ins, const char *input_word = "an input") {
    const AliasPair hit = first_alias(outs.begin(), (int)outs.size(), ins.begin(), (int)ins.size());
    if (hit.out < 0) return 0;
    const char *name = outs.begin()[hit.out].name;
    return hit.input ? fail(-2, "%s may not alias %s", name, input_word) : fail(-2, "%s and %s may not alias each other", name, outs.begin()[hit.other].name);
}
// (rtw_render_host.hip and rtw_stage_host.hip define the host-buffer entry points of the C ABI themselves: nothing of them is declared here)

// rtw_multi.hip
int ensure_peer(const CtxPtr &ctx, int dev, int root, bool *direct);
struct RcclSet;                                               // the communicators of one device list (one rank per device)
int rccl_acquire(const std::vector<int> &devs, std::shared_ptr<RcclSet> *out, std::unique_lock<std::mutex> *use);
int rccl_reduce_frames(RcclSet &set, const std::vector<const void *> &send, void *recv_root, size_t count, bool f64, const std::vector<hipStream_t> &streams);
void rccl_shutdown();
int launch_untile(bool f64, const void *gather, void *frame, int W, int H, long n_tiles, int n_shards, long pad_tiles, hipStream_t stream);

// rtw_accum_kernels.hip: the unit ops 21-23, 25, 30, 31 (include/rtw_hip.h rtw_unit_f32 / _f64): the accumulator's kernels on the caller's
// words, through the launches the host paths themselves use
int accum_unit(int op, bool f64, int count, const void *in, void *out);
// rtw_accum.hip: an accumulator as the denoiser's input -- what rtw_accum_features_* / rtw_accum_noise_* run and what rtw_accum_filtered_*
// (rtw_render_host.hip) strings together.  validate_*: every refusal, before any HIP call; enqueue_*: wait for the accumulator's event,
// launch on `stream`, record the event (everything reads the words and C_t only).
// (the templates on CamT: rtw_camera_f32 or rtw_camera_f64, instantiated for both in rtw_accum.hip)
template <typename CamT> int validate_accum_features(rtw_scene_handle scene, const CamT *cam, const rtw_params *p, rtw_accum_handle a);
template <typename CamT> int enqueue_accum_features(rtw_scene_handle scene, const CamT *cam, const rtw_params *p, rtw_accum_handle a, void *d_out, hipStream_t stream, RenderRec **rec, CtxPtr *ctx);
int accum_device_of(rtw_accum_handle a);
bool accum_is_adaptive(rtw_accum_handle a);
int validate_accum_noise(rtw_accum_handle a, bool f64);                                             // adaptive, its last call finished, the call's precision
int enqueue_accum_noise(rtw_accum_handle a, bool f64, void *d_out, hipStream_t stream);               // H*W elements of T
int enqueue_accum_resolve(rtw_accum_handle a, bool f64, int32_t gamma, void *d_out, hipStream_t stream);   // rtw_accum_resolve_*'s own path
// ... and the batched forms (rtw_accum_resolve_batch_* / _features_batch_* / _noise_batch_*, strung together by rtw_accum_filtered_batch_*): n_views >= 1
// accumulators of one size on one device, ONE launch per pass.  validate_accum_array: a null array or entry, the count -- an entry point calls
// it once, first.  validate_*_batch: every refusal that looks at a handle (a handle given twice, every view as the single call validates it,
// the batch's own rules), before any HIP call; enqueue_*: wait for EVERY accumulator's
// event, launch on `stream`, record every event.  Frames lie view-major behind d_out.
int validate_accum_array(const rtw_accum_handle *accums, int32_t n_views);
template <typename CamT> int validate_accum_features_batch(rtw_scene_handle scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_accum_handle *accums);
template <typename CamT> int enqueue_accum_features_batch(rtw_scene_handle scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_accum_handle *accums, void *d_out, hipStream_t stream, RenderRec **rec, CtxPtr *ctx);
int validate_accum_noise_batch(const rtw_accum_handle *accums, int32_t n_views, bool f64);
int enqueue_accum_noise_batch(const rtw_accum_handle *accums, int32_t n_views, bool f64, void *d_out, hipStream_t stream);
int validate_accum_resolve_batch(const rtw_accum_handle *accums, int32_t n_views, bool f64);
int enqueue_accum_resolve_batch(const rtw_accum_handle *accums, int32_t n_views, bool f64, int32_t gamma, void *d_out, hipStream_t stream);

// rtw_features.hip -- first-hit feature buffers (include/rtw_hip.h rtw_render_features_*).  validate_features: the checks that need no device
// (the render, whole frames on one device, the chunk range); validate_features_batch: validate_batch's rules together with those and a tile
// count the one launch can number.
int validate_features(const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, int *n_chunks, int *chunk_spp);
int validate_features_batch(const void *cams, int32_t n_views, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, const void *out, int *n_chunks, int *chunk_spp);
// launch_features: enqueue the feature kernel for the chunks [chunk_begin, chunk_begin + chunk_count) on `stream`, `rec` receives the counters
// and the kernel's events like a render's.  n_views as for launch_render: 0 -- the one camera `cams` points to; >= 1 -- ONE launch of a BATCH
// instance for that many cameras, seeds (null: p->seed) and buffers of W*H*8 elements behind d_out.
// d_tile_chunks non-null (n_views == 0 only): the pass over what an adaptive accumulator holds -- tile t gets the chunks [0, d_tile_chunks[t])
// (device memory, the accumulator's C_t array), the call's own range is validated and otherwise unused.
// view_tiles non-null (n_views >= 1 only): the same pass for a batch of adaptive accumulators in ONE launch of a TILED && BATCH instance -- a HOST
// array of n_views such device arrays, tile t of view v gets the chunks [0, view_tiles[v][t]).
template <typename T, typename CamT>
int launch_features(rtw_scene_handle scene, const CamT *cams, int n_views, const uint64_t *seeds, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, void *d_out, hipStream_t stream, RenderRec **rec_out, CtxPtr *ctx_out, const int *d_tile_chunks = nullptr, const int *const *view_tiles = nullptr);
// rtw_features_accum_batch_f32.hip / _f64.hip: the TILED && BATCH instance of the feature kernel for a scan variant, as launch_features chooses
// among the other instances (`fixed`: the headline variant with the default numerics mode compiled in)
const void *features_tiled_batch_kernel_f32(bool mfma, bool lds_scene, bool fixed);
const void *features_tiled_batch_kernel_f64(bool mfma, bool lds_scene, bool fixed);

// rtw_rays.hip -- ray queries (include/rtw_hip.h rtw_cast_rays_*).  validate_rays: every check of a call that needs neither a device nor a
// pointer -- the parameters and the count (n == 0 passes: the caller returns 0 without a launch).  launch_rays: enqueue the ray kernel (ONE
// launch) for n >= 1 rays on `stream`, `rec` receives the counters and the kernel's events like a render's; d_rays / d_rec (null: no records)
// 16-byte, d_idx 4-byte aligned DEVICE pointers.
int validate_rays(const rtw_rays_params *p, int64_t n);
template <typename T>
int launch_rays(rtw_scene_handle scene, const void *d_rays, int64_t n, const rtw_rays_params *p, void *d_idx, void *d_rec, hipStream_t stream, RenderRec **rec_out, CtxPtr *ctx_out);

// rtw_trace_rays.hip -- radiance queries (include/rtw_hip.h rtw_trace_rays_*).  validate_trace_rays: every check of a call that needs neither
// a device nor a pointer -- the parameters, the count and the two 64-bit ranges (n == 0 passes: the caller returns 0 without a launch).
// launch_trace_rays: enqueue the radiance kernel (ONE launch) for n >= 1 rays on `stream`, `rec` receives the counters and the kernel's
// events like a render's; d_rays 16-byte, d_out (n x 3 binary64) 8-byte aligned DEVICE pointers.
int validate_trace_rays(const rtw_trace_params *p, int64_t n);
template <typename T>
int launch_trace_rays(rtw_scene_handle scene, const void *d_rays, int64_t n, const rtw_trace_params *p, void *d_out, hipStream_t stream, RenderRec **rec_out, CtxPtr *ctx_out);

// rtw_denoise.hip -- the feature-guided denoiser (include/rtw_hip.h rtw_denoise_*, rtw_filter_batch_*).  validate_denoise: the checks of one
// frame that need no device; validate_filter_batch: those, n_views and the batch's size.
int validate_denoise(const rtw_denoise_t *d, int32_t width, int32_t height);
int validate_filter_batch(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views);
// launch_denoise: enqueue its kernels on `stream` of the current device.  n_views == 0: one frame, d_work of rtw_denoise_work_bytes bytes
// (16-byte aligned); d_noise non-null: the noise-guided form (rtw_guided_filter_device_*), H*W elements of T, the per-pixel relative noise.
// n_views >= 1: that many frames of one size in prepare + `levels` launches; every buffer (d_noise: n_views*H*W elements) and every plane of the
// workspace (n_views * rtw_denoise_work_bytes bytes) holds the views one behind the other.
template <typename T>
int launch_denoise(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views, const void *d_image, const void *d_features, void *d_out, void *d_work, hipStream_t stream, const void *d_noise = nullptr);

// rtw_upsample.hip -- the feature-guided upsampler (include/rtw_hip.h rtw_upsample_*).  validate_upsample: every check of a call that needs no
// device -- the parameters, both frame sizes, n_views (0: one frame) and the batch's size.
int validate_upsample(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, int32_t n_views, int elem_bytes);
// launch_upsample: enqueue prepare + `levels` level passes at the small size and the upsampling kernel at the full size on `stream` of the current
// device.  n_views == 0: one frame, d_work of rtw_upsample_work_bytes bytes (16-byte aligned); n_views >= 1: that many views in the same number
// of launches, every buffer and every plane of the workspace (n_views times the bytes) holds the views one behind the other, each at its own size.
template <typename T>
int launch_upsample(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, int32_t n_views, const void *d_image_lo, const void *d_features_lo, const void *d_features_hi, void *d_out, void *d_work, hipStream_t stream);

// rtw_temporal.hip -- temporal reprojection (include/rtw_hip.h rtw_temporal_*).  validate_temporal: every check of a step that needs neither a
// device nor a pointer -- the parameters and the frame.
int validate_temporal(const rtw_temporal_t *t, int32_t width, int32_t height, int elem_bytes);
// launch_temporal: enqueue ONE step (one launch) on `stream` of the current device.  n_paths == 0: ONE path -- cam_prev and d_state_prev are
// both null (the first frame) or both given; the states hold rtw_temporal_state_bytes bytes each (16-byte aligned).  n_paths >= 1
// (rtw_reproject_batch_device_*): that many paths in the same ONE launch -- cam / cam_prev are unused, path s takes its constants from entry s of
// the DEVICE table d_table (temporal_table: 32 elements of T per path) and every buffer holds the paths one behind the other; d_state_prev
// null: every path's first frame.  d_moment_next non-null: the step with moments
// (rtw_history_moments_*), planes of rtw_history_moment_bytes bytes, d_moment_prev null exactly when d_state_prev is.  `c` non-null (accepted by
// validate_temporal_clamp: every check of a clamp, none needs a device): the clamped step (rtw_clamped_step_*), still one launch.
int validate_temporal_clamp(const rtw_temporal_clamp_t *c);
template <typename T, typename CamT>
int launch_temporal(const rtw_temporal_t *t, const CamT *cam, const CamT *cam_prev, int32_t n_paths, const void *d_table, int32_t width, int32_t height, const void *d_image, const void *d_features, const void *d_state_prev, void *d_state_next, void *d_out, hipStream_t stream, const void *d_moment_prev = nullptr, void *d_moment_next = nullptr, const rtw_temporal_clamp_t *c = nullptr, const void *d_motion = nullptr);
// temporal_table: the camera constants of n paths into a HOST table, 32 elements per path (include/rtw_hip.h rtw_reproject_table_*; cams_prev null: first
// frames) -- the one copy of that arithmetic, launch_temporal's own constants included.
template <typename T, typename CamT> void temporal_table(const CamT *cams, const CamT *cams_prev, int64_t n, T *table);
// validate_temporal_noise: every check of a noise map (rtw_history_noise_device_*) that needs neither a device nor a pointer.  launch_temporal_noise:
// enqueue the map (ONE launch) of a state and its moment plane on `stream` of the current device; d_noise: width*height elements of T.
// n_paths >= 1 (rtw_reproject_noise_batch_device_*): the maps of that many states and planes, one behind the other, in the same ONE launch.
int validate_temporal_noise(const rtw_temporal_noise_t *n, int32_t width, int32_t height, int elem_bytes);
template <typename T> int launch_temporal_noise(const rtw_temporal_noise_t *n, int32_t width, int32_t height, int32_t n_paths, const void *d_state, const void *d_moment, void *d_noise, hipStream_t stream);

// rtw_motion.hip -- the first-hit motion pass (include/rtw_hip.h rtw_first_hit_motion_*).  validate_motion: every check of a pass that needs
// neither a device nor a pointer (of `p`: the frame, the device, the flag bits).  launch_motion: enqueue the pass (ONE launch, no record) on
// `stream` of the scene's device, which must be current; d_table (scene->n rows of 4 elements, or null: m = 0) and d_motion (width*height
// slots of 4 elements) are 16-byte aligned DEVICE pointers.
int validate_motion(const rtw_params *p, int elem_bytes);
template <typename T, typename CamT> int launch_motion(rtw_scene_handle scene, const CamT *cam, const rtw_params *p, const void *d_table, void *d_motion, hipStream_t stream);
// motion_table: the body of rtw_motion_table_* (include/rtw_hip.h), a frame's table into HOST memory
template <typename T, typename SceneT> int motion_table(const SceneT *prev, const SceneT *cur, T *table);

// rtw_motion_blur.hip -- the motion-blur stage (include/rtw_hip.h rtw_velocity_blur_*).  validate_motion_blur: every check of a blur that needs
// neither a device nor a pointer.  launch_motion_blur: enqueue the stage (THREE launches, no record) on `stream` of the current device; d_work:
// rtw_velocity_blur_work_bytes bytes.  cam_prev null (frame 0 of rtw_render_blurred_*): ONE launch, the image passes through with the
// gamma applied; d_motion and d_work are not looked at.
int validate_motion_blur(const rtw_velocity_blur_t *b, int32_t width, int32_t height, int elem_bytes);
template <typename T, typename CamT>
int launch_motion_blur(const rtw_velocity_blur_t *b, const CamT *cam, const CamT *cam_prev, int32_t width, int32_t height, const void *d_image, const void *d_features, const void *d_motion, void *d_work, void *d_out, hipStream_t stream);

// ---- the lens family: rtw_defocus_*, rtw_wide_aperture_*, rtw_lens_batch_* (include/rtw_hip.h) -----------------------------------------
// The three stages are one: the wide-aperture stage with max_radius <= 8 IS the defocus stage, and the batch runs the same launches over N
// views.  Each tier of entry points has ONE body -- lens_device (rtw_wide_aperture.hip), lens_host (rtw_stage_host.hip), render_host_lens
// (rtw_render_host.hip) -- that takes `top`, the stage's largest max_radius (8 or 32), and n_views: 0 for the single forms, which then run
// without a table and with a null LensViews.  The bodies take rtw_wide_aperture_t; the two stages' parameter structs have the same fields in
// the same order, and an rtw_defocus_* entry point hands its own over through this copy (null stays null).
static_assert(sizeof(rtw_wide_aperture_t) == sizeof(rtw_defocus_t) && sizeof(rtw_wide_aperture_t) == 40, "the two stages' parameters have the same fields");
struct AsWideAperture {
    rtw_wide_aperture_t copy;
    const rtw_wide_aperture_t *ptr;
    explicit AsWideAperture(const rtw_defocus_t *b) : ptr(b ? &copy : nullptr) { if (b) memcpy(&copy, b, sizeof copy); }
};
// rtw_lens_batch_* and rtw_lens_batch_device_* NAME the count they refuse, so batch_views' -1 will not do for them: they hand their
// caller's count down as it is but for 0 -- below the ABI the single form --, which goes down as LENS_NO_VIEWS and is refused and named
// as the 0 it was (validate_lens_batch_frame).
constexpr int32_t LENS_NO_VIEWS = std::numeric_limits<int32_t>::min();
inline int32_t lens_batch_views(int32_t n_views) { return n_views ? n_views : LENS_NO_VIEWS; }

// rtw_defocus.hip -- the defocus stage and the family's checks of ONE view.  validate_lens: every check that needs neither a device nor a
// pointer, in four parts in this order -- the parameters (check_lens_params: max_radius in 1..top, flags, gamma, device, reserved), the
// lens (lens_radius, focus_dist), the frame (check_lens_frame: the sizes, then the denoiser's frame rule) and the camera (its horizontal
// extent and focus plane).  launch_defocus: enqueue the stage (TWO launches, no record) on `stream` of the current device; d_work:
// rtw_defocus_work_bytes bytes.  The camera's lens_radius is not read: the aperture is b->lens_radius.
template <typename CamT> int validate_lens(const rtw_defocus_t *b, const CamT *cam, int32_t width, int32_t height, int top);
int check_lens_params(const rtw_defocus_t *b, int top);
int check_lens_frame(int32_t width, int32_t height, int elem_bytes);
// A batch of views for the lens stages (rtw_lens_batch_*; rtw_layout.hpp LensBatchLayout has the arithmetic): n_views >= 1 views in each
// launch, view v's lens in entry v of the DEVICE table d_table (lens_table_entry), its image, features, workspace and output v strides (BYTES)
// behind the pointers; an input stride of 0: every view reads the one frame.  Below the ABI a null LensViews is the single call.
struct LensViews { int32_t n_views; const void *d_table; long long img_stride, feat_stride, work_stride, out_stride; };
inline LensViews lens_views(const LensBatchLayout &R, int32_t n_views, const void *d_table) {
    return {n_views, d_table, (long long)R.img_stride, (long long)R.feat_stride, (long long)R.work_stride, (long long)R.out_stride};
}
template <typename T, typename CamT>
int launch_defocus(const rtw_defocus_t *b, const CamT *cam, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_work, void *d_out, hipStream_t stream, const LensViews *vb = nullptr);
// Its two launches one by one, for the wide-aperture stage: launch_defocus_prepare is the prepare launch with the clamp `rm` (b->max_radius is not read) into a CoC plane and its tile plane;
// launch_defocus_gather is the gather of a frame of any size over an image, a CoC plane and a tile plane, mmax (1..8) >= every radius there.
// n_views == 0: one view.  n_views >= 1: that many views in the same ONE launch; `strides`: four byte strides from one view to the next, one
// per pointer in the order of the arguments; the prepare launch then reads neither b nor cam but entry v of the device table d_table.
template <typename T, typename CamT>
int launch_defocus_prepare(const rtw_defocus_t *b, int rm, const CamT *cam, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_coc, void *d_tile, hipStream_t stream, int32_t n_views = 0, const void *d_table = nullptr, const long long *strides = nullptr);
template <typename T>
int launch_defocus_gather(int32_t width, int32_t height, int mmax, int gamma, const void *d_image, const void *d_coc, const void *d_tile, void *d_out, hipStream_t stream, int32_t n_views = 0, const long long *strides = nullptr);
dim3 lens_views_grid(unsigned tiles, int32_t n_views);       // the grid of a batched lens launch: the tiles of one view in x, the views over y and z
// one view's entry of the lens table (include/rtw_hip.h rtw_lens_table_*; b: lens_radius and focus_dist alone are read): the one copy of that arithmetic
template <typename T, typename CamT> void lens_table_entry(const rtw_defocus_t *b, const CamT *cam, int32_t width, T *e);

// rtw_wide_aperture.hip -- the wide-aperture stage (include/rtw_hip.h rtw_wide_aperture_*): circles of confusion up to 32 px through a reduced
// copy of the frame.  launch_wide_aperture: enqueue the stage (SIX launches, or the defocus stage's two when max_radius <= 8 -- what the
// defocus stage's own entry points run; no record) on `stream` of the
// current device; d_work: rtw_wide_aperture_work_bytes bytes.  vb non-null (rtw_lens_batch_*): vb->n_views views in the same launches.
template <typename T, typename CamT>
int launch_wide_aperture(const rtw_wide_aperture_t *b, const CamT *cam, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_work, void *d_out, hipStream_t stream, const LensViews *vb = nullptr);
// The checks of n_views >= 1 views that need neither a device nor a pointer (every entry point of the family but the batched device
// form; a single form: ONE view without arrays): the count, then per view validate_lens with lens_radii[v] / focus_dists[v] (null arrays:
// b's own) and max_radius in 1..top -- the first offending view is named, unless it is one view without arrays --, then the batch's size
// (-5; one view never reaches it: the frame rule is the narrower).  own_lens (the one-call forms alone): a lens radius of -1 is cams[v]'s
// own.  `lens_out` non-null: n_views rtw_defocus_t with every view's lens radius and focus distance in place.
template <typename CamT>
int validate_lens_batch(const rtw_wide_aperture_t *b, const CamT *cams, int32_t n_views, int32_t width, int32_t height, const double *lens_radii, const double *focus_dists, bool own_lens, int top, std::vector<rtw_defocus_t> *lens_out);
// the lens table of those views into a HOST table (32 elements per view)
template <typename T, typename CamT> void lens_table(const std::vector<rtw_defocus_t> &lens, const CamT *cams, int32_t width, T *table);
// what a batched entry point checks of its counts and frame without a camera: the counts, check_lens_params with top 32, check_lens_frame, the batch's size
int validate_lens_batch_frame(const rtw_wide_aperture_t *b, int32_t n_views, int32_t n_frames, int32_t width, int32_t height, int elem_bytes);

// rtw_present.hip -- the present stage (include/rtw_hip.h rtw_present_*).  validate_present: every check of a call that needs neither a device
// nor a pointer -- the parameters, the frame, n_views (0: one frame; a batch's count through batch_views) and the size of the launch.
int validate_present(const rtw_present_t *p, int32_t width, int32_t height, int32_t n_views);
// launch_present: enqueue ONE launch on `stream` of the current device.  n_views == 0: one frame of width*height*3 elements into
// width*height*channels bytes (d_out 4-byte aligned); n_views >= 1: that many frames one behind the other in both buffers.
template <typename T> int launch_present(const rtw_present_t *p, int32_t width, int32_t height, int32_t n_views, const void *d_images, void *d_out, hipStream_t stream);

// rtw_unit.hip
template <typename T, typename SceneT, typename CamT> int run_unit(int op, int count, const void *in, void *out, const SceneT *scene, const CamT *cam);

}  // namespace rtwh

#pragma GCC visibility pop
