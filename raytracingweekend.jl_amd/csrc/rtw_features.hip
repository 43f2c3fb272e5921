// rtw_features.hip -- first-hit feature buffers (include/rtw_hip.h rtw_render_features_*): the checks that need no device, ONE launch of the
// feature kernel (rtw_features.hpp) per call -- its own parameters, instance and grid; camera, numerics mode and scene view (rtw_scene_view.hpp) and the
// record sequence (rtw_host.hpp begin_record / run_record) are the ones launch_render (rtw_launch.hip) uses --, and the device-resident entry points.
// n_views == 0 is the single-view call; n_views >= 1 (rtw_render_features_batch_*) the same launch with a BATCH instance over that many views,
// whose cameras and seeds go up with the record (upload_views, rtw_launch.hip).
// (The host-buffer entry points live with the other cached-context paths in rtw_render_host.hip.)
#include "rtw_scene_view.hpp"
#include "rtw_features.hpp"

namespace rtwh {

// Everything about a feature render that is decided without a device: the render's own parameters, whole frames on one device, the chunk
// range in units of the render's effective chunks.
int validate_features(const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, int *n_chunks, int *chunk_spp) {
    int nch, cs;
    if (int rc = validate_params(p, &nch, &cs)) return rc;
    if (p->shard_count != 1) return fail(-2, "a feature render renders whole frames (shard_count = %d)", p->shard_count);
    if (p->flags & RTW_FLAG_COMPACT_TILES) return fail(-2, "a feature render writes whole frames (RTW_FLAG_COMPACT_TILES is a per-shard layout)");
    if (p->flags & RTW_FLAG_RCCL_REDUCE) return fail(-2, "a feature render runs on one device (RTW_FLAG_RCCL_REDUCE)");
    if (p->flags & RTW_FLAG_RAY_POOL) return fail(-2, "a feature render runs its own kernel (RTW_FLAG_RAY_POOL)");
    if (p->n_devices > 1 || p->n_devices < 0 || p->device_ids)
        return fail(-2, "a feature render runs on one device (n_devices = %d%s)", p->n_devices, p->device_ids ? ", device_ids given" : "");
    if (p->job_pixels != 0 && p->job_pixels != 1 && p->job_pixels != 4 && p->job_pixels != 8 && p->job_pixels != 16)
        return fail(-2, "job_pixels must be 0 (automatic), 1, 4, 8 or 16");
    if (int rc = check_chunk_range(chunk_begin, chunk_count, nch)) return rc;
    const long long n_tiles = (long long)((p->height + 7) / 8) * ((p->width + 7) / 8);
    if (n_tiles >= (1ll << 31)) return fail(-5, "render too large for one call: %lld tiles", n_tiles);
    *n_chunks = nch; *chunk_spp = cs;
    return 0;
}

// A batched feature render (rtw_render_features_batch_*): validate_batch's rules together with validate_features'.  What the one launch
// must be able to number -- the batch's tiles (flat, v * n_tiles + t) and its workgroups -- is inside validate_batch's bound for the render's
// queues (n_views x tiles < 2^28); the check below states it for this launch.
int validate_features_batch(const void *cams, int32_t n_views, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, const void *out, int *n_chunks, int *chunk_spp) {
    if (int rc = validate_batch(cams, n_views, p, out)) return rc;
    if (int rc = validate_features(p, chunk_begin, chunk_count, n_chunks, chunk_spp)) return rc;
    const long long n_tiles = (long long)((p->height + 7) / 8) * ((p->width + 7) / 8);
    if ((double)n_tiles * (double)n_views >= (double)(1ll << 31)) return fail(-5, "batch too large for one call: %d views of %lld tiles", n_views, n_tiles);
    return 0;
}

// Enqueue the feature kernel for the chunks [chunk_begin, chunk_begin + chunk_count) of the render `p` describes (validate_features has
// accepted them) on `stream`; `rec` receives the counters and the kernel's events like a render's.
// d_tile_chunks non-null (rtw_accum_features_* on an adaptive accumulator, rtw_accum.hip): the TILED instances -- tile t gets the chunks
// [0, d_tile_chunks[t]) instead of the call's range (which the caller passes as [0, 1): validated, not looked at by the kernel).
// n_views >= 1 (validate_features_batch has accepted it; no d_tile_chunks): ONE launch of a BATCH instance over the n_views cameras `cam`
// points to, `seeds` (null: p->seed for every view) and n_views buffers behind d_out; the views go up with the record (upload_views).
// view_tiles non-null (n_views >= 1 only; rtw_accum_features_batch_* on adaptive accumulators): a HOST array of n_views device pointers, the
// accumulators' tile-chunk arrays -- ONE launch of a TILED && BATCH instance (rtw_features_accum_batch_f32.hip / _f64.hip), the table goes up with the views.
template <typename T> const void *features_tiled_batch_kernel(bool mfma, bool lds_scene, bool fixed);
template <> const void *features_tiled_batch_kernel<float>(bool mfma, bool lds_scene, bool fixed) { return features_tiled_batch_kernel_f32(mfma, lds_scene, fixed); }
template <> const void *features_tiled_batch_kernel<double>(bool mfma, bool lds_scene, bool fixed) { return features_tiled_batch_kernel_f64(mfma, lds_scene, fixed); }

// The feature kernel's instances over the scan (matrix pipe or VALU) and where the scene lives (LDS or global memory), written once for the
// plain, the TILED and the BATCH form (TILED && BATCH: the same table in a unit per precision, rtw_features_accum_batch_f32.hip / _f64.hip).  FIXED (mfma && lds_scene): the one instance with the default numerics mode compiled in.
template <typename T, bool TILED, bool BATCH, bool FIXED = false>
const void *feature_instance(bool mfma, bool lds_scene) {
    if constexpr (FIXED) return (const void *)rtw::features_kernel<T, true, true, rtw::NUM_REFERENCE, TILED, BATCH>;
    if (mfma) return lds_scene ? (const void *)rtw::features_kernel<T, true, true, -1, TILED, BATCH> : (const void *)rtw::features_kernel<T, true, false, -1, TILED, BATCH>;
    return lds_scene ? (const void *)rtw::features_kernel<T, false, true, -1, TILED, BATCH> : (const void *)rtw::features_kernel<T, false, false, -1, TILED, BATCH>;
}

template <typename T, typename CamT>
int launch_features(rtw_scene_handle scene, const CamT *cam, int n_views, const uint64_t *seeds, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, void *d_out,
                    hipStream_t stream, RenderRec **rec_out, CtxPtr *ctx_out, const int *d_tile_chunks, const int *const *view_tiles) {
    if (!scene || !cam || !p || !d_out) return fail(-1, "null argument");
    const bool batch = n_views != 0;
    if (batch ? d_tile_chunks != nullptr : view_tiles != nullptr) return fail(-9, "internal: a batch takes its tile-chunk arrays as a table, a single view as one array");
    int nch, cs;
    if (batch) { if (int rc = validate_features_batch(cam, n_views, p, chunk_begin, chunk_count, d_out, &nch, &cs)) return rc; }
    else if (int rc = validate_features(p, chunk_begin, chunk_count, &nch, &cs)) return rc;
    if (((uintptr_t)d_out & 15u) != 0) return fail(-2, "the feature buffer must be 16-byte aligned");
    if (scene->is_f64 != (sizeof(T) == 8)) return fail(-4, "scene handle precision does not match the call");
    if (p->device >= 0 && p->device != scene->device)
        return fail(-4, "params.device %d != scene device %d", p->device, scene->device);
    CtxPtr ctx;
    if (int rc = get_ctx(scene->device, &ctx)) return rc;
    *ctx_out = ctx;
    HIP_TRY(hipSetDevice(scene->device));

    rtw::FeatParams K;
    memset(&K, 0, sizeof K);
    K.width = p->width; K.height = p->height; K.spp = p->spp; K.chunk_spp = cs;
    K.chunk_begin = chunk_begin; K.chunk_count = chunk_count;
    K.tiles_i = (p->height + 7) / 8;
    K.n_tiles = (unsigned)((long long)K.tiles_i * ((p->width + 7) / 8));
    K.seed = p->seed;
    const rtw::Camera<T> C = device_camera<T>(*cam);
    // the scans of the trace kernel's plain render (rtw_launch.hip): pass 1 on the matrix pipe over the plain scan's own sphere order, or,
    // under RTW_FLAG_SCAN_VALU and for scenes without the operands, the all-VALU scan over the caller's order.  RTW_FLAG_GROUP_CULL is
    // accepted and runs the same scans: the words are the same by definition, and the cull layout has not been measured on primary rays.
    const int numerics = numerics_of(p->flags);
    const bool mfma = scene->mf_ops != nullptr && !(p->flags & RTW_FLAG_SCAN_VALU);
    PlainView<T> V;
    if (int rc = plain_scene_view<T>(scene, mfma, numerics, &V)) return rc;
    const size_t lds_bytes = (batch ? rtw::feat_fixed_lds_bytes<T, true>() : rtw::feat_fixed_lds_bytes<T>()) + (V.lds_scene ? V.scene_bytes : 0);
    const bool tiled = d_tile_chunks != nullptr || view_tiles != nullptr;
    // the default numerics mode of the headline variant (scene in LDS, matrix pipe): the mode fixed at compile time
    const bool fixed = mfma && V.lds_scene && numerics == rtw::NUM_REFERENCE;
    const void *kern = batch ? feature_instance<T, false, true>(mfma, V.lds_scene) : !tiled ? feature_instance<T, false, false>(mfma, V.lds_scene) : feature_instance<T, true, false>(mfma, V.lds_scene);
    // (asked for after the table, so that the instances are emitted in the order they always were and the object's device code stays the same bytes)
    if (fixed) kern = batch ? feature_instance<T, false, true, true>(mfma, V.lds_scene) : tiled ? feature_instance<T, true, false, true>(mfma, V.lds_scene) : feature_instance<T, false, false, true>(mfma, V.lds_scene);
    if (batch && tiled) kern = features_tiled_batch_kernel<T>(mfma, V.lds_scene, fixed);
    // (a batch: its tiles numbered flat, v * n_tiles + t -- validate_features_batch: fewer than 2^31)
    const unsigned total_tiles = batch ? K.n_tiles * (unsigned)n_views : K.n_tiles;
    const unsigned grid = (total_tiles + RTW_FEATURE_WAVES - 1u) / RTW_FEATURE_WAVES;
    // (test aid: which instance the rules above picked, in the form of the trace kernel's line -- rtw_launch.hip; the grid is one workgroup
    //  per RTW_FEATURE_WAVES tiles, no occupancy question is asked: blocks_per_cu=0)
    static const bool debug = aid_env("RTW_DEBUG") != nullptr;
    if (debug) {
        char views[32] = "";                                                    // (the TILED && BATCH instance alone: " views=N" at the end of the line)
        if (batch && tiled) snprintf(views, sizeof views, " views=%d", n_views);
        fprintf(stderr, "[rtw debug] features instance: %s lds_scene=%d cull=0 mfma=%d fixed=%d batch=%d accum=%d adapt=%d lds_bytes=%zu blocks_per_cu=0%s\n", sizeof(T) == 8 ? "f64" : "f32",
                (int)V.lds_scene, (int)mfma, (int)fixed, (int)batch, (int)tiled, (int)tiled, lds_bytes, views);
    }

    if (int rc = begin_record(ctx.get(), scene, nch, (int)grid, 64 * RTW_FEATURE_WAVES, offsetof(rtw::DevCounters, t_first), stream, rec_out)) return rc;
    rtw::FeatTiledViews<T> FV;          // (a BATCH instance that is not TILED takes its base, rtw::FeatViews<T>: the same bytes in front)
    memset(&FV, 0, sizeof FV);
    if (batch) {
        const void *d_cams = nullptr;
        if (int rc = upload_views<T>(*rec_out, cam, n_views, seeds, p->seed, stream, &d_cams, &FV.seeds, view_tiles, &FV.chunks)) return rc;
        FV.cams = (const rtw::Camera<T> *)d_cams;
        FV.total_tiles = total_tiles;
        FV.view_elems = (unsigned long long)p->width * (unsigned long long)p->height * RTW_FEATURE_CHANNELS;
    }
    // the kernel's last argument (rtw::FeatLastArg): the views of a BATCH instance, else the tiles' chunk counts (null but for a TILED one)
    void *args[] = {&K, (void *)&C, &V.scene, &d_out, &(*rec_out)->ctr, batch ? (void *)&FV : (void *)&d_tile_chunks};
    return run_record(*rec_out, stream, [&] { (void)hipLaunchKernel(kern, dim3(grid), dim3(64 * RTW_FEATURE_WAVES), args, lds_bytes, stream); });
}

// The device-resident entry points rtw_render_features_device_* (n_views == 0) and rtw_render_features_batch_device_* (n_views != 0).
template <typename T, typename CamT>
int features_device(rtw_scene_handle scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, void *d_out,
                    void *stream_v) {
    if (!p) return fail(-1, "null params");
    if (!scene || !cams || !d_out) return fail(-1, "null argument");
    int nch, cs;
    if (int rc = n_views ? validate_features_batch(cams, n_views, p, chunk_begin, chunk_count, d_out, &nch, &cs) : validate_features(p, chunk_begin, chunk_count, &nch, &cs)) return rc;
    if (((uintptr_t)d_out & 15u) != 0) return fail(-2, "the feature buffer must be 16-byte aligned");
    DeviceGuard guard;
    RenderRec *rec = nullptr;
    CtxPtr ctx;
    release_last();
    int rc = launch_features<T>(scene, cams, n_views, seeds, p, chunk_begin, chunk_count, d_out, (hipStream_t)stream_v, &rec, &ctx);
    hold_last(rec, ctx);               // (also on a late error: released by the next call)
    return rc;
}

template int launch_features<float>(rtw_scene_handle, const rtw_camera_f32 *, int, const uint64_t *, const rtw_params *, int32_t, int32_t, void *, hipStream_t, RenderRec **, CtxPtr *, const int *, const int *const *);
template int launch_features<double>(rtw_scene_handle, const rtw_camera_f64 *, int, const uint64_t *, const rtw_params *, int32_t, int32_t, void *, hipStream_t, RenderRec **, CtxPtr *, const int *, const int *const *);

}  // namespace rtwh

using namespace rtwh;

extern "C" {

int rtw_render_features_device_f32(rtw_scene_handle s, const rtw_camera_f32 *c, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, void *d_out, void *stream) {
    return features_device<float>(s, c, 0, nullptr, p, chunk_begin, chunk_count, d_out, stream);
}
int rtw_render_features_device_f64(rtw_scene_handle s, const rtw_camera_f64 *c, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, void *d_out, void *stream) {
    return features_device<double>(s, c, 0, nullptr, p, chunk_begin, chunk_count, d_out, stream);
}
int rtw_render_features_batch_device_f32(rtw_scene_handle s, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, int32_t chunk_begin,
                                         int32_t chunk_count, void *d_out, void *stream) {
    return features_device<float>(s, cams, batch_views(n_views), seeds, p, chunk_begin, chunk_count, d_out, stream);
}
int rtw_render_features_batch_device_f64(rtw_scene_handle s, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, int32_t chunk_begin,
                                         int32_t chunk_count, void *d_out, void *stream) {
    return features_device<double>(s, cams, batch_views(n_views), seeds, p, chunk_begin, chunk_count, d_out, stream);
}

}  // extern "C"
