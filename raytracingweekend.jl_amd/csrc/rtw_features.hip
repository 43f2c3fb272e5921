// rtw_features.hip -- first-hit feature buffers (include/rtw_hip.h rtw_render_features_*): the checks that need no device, ONE launch of the
// feature kernel (rtw_features.hpp) per call with the render records and events every render uses, and the device-resident entry points.
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
    if (chunk_begin < 0 || chunk_count < 1 || (long long)chunk_begin + chunk_count > nch)
        return fail(-2, "chunk range [%d, %lld) is not inside the render's %d chunks", chunk_begin, (long long)chunk_begin + chunk_count, nch);
    const long long n_tiles = (long long)((p->height + 7) / 8) * ((p->width + 7) / 8);
    if (n_tiles >= (1ll << 31)) return fail(-5, "render too large for one call: %lld tiles", n_tiles);
    *n_chunks = nch; *chunk_spp = cs;
    return 0;
}

// Enqueue the feature kernel for the chunks [chunk_begin, chunk_begin + chunk_count) of the render `p` describes (validate_features has
// accepted them) on `stream`; `rec` receives the counters and the kernel's events like a render's.
template <typename T, typename CamT>
int launch_features(rtw_scene_handle scene, const CamT *cam, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, void *d_out, hipStream_t stream,
                    RenderRec **rec_out, CtxPtr *ctx_out) {
    if (!scene || !cam || !p || !d_out) return fail(-1, "null argument");
    int nch, cs;
    if (int rc = validate_features(p, chunk_begin, chunk_count, &nch, &cs)) return rc;
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
    rtw::Camera<T> C;
    for (int k = 0; k < 3; ++k) {
        C.origin[k] = cam->origin[k]; C.llc[k] = cam->lower_left_corner[k];
        C.horizontal[k] = cam->horizontal[k]; C.vertical[k] = cam->vertical[k];
        C.u[k] = cam->u[k]; C.v[k] = cam->v[k]; C.w[k] = cam->w[k];
    }
    C.lens_radius = cam->lens_radius;
    using V4 = typename rtw::Vec4<T>::type;
    // the scans of the trace kernel's plain render (rtw_launch.hip): pass 1 on the matrix pipe over the plain scan's own sphere order, or,
    // under RTW_FLAG_SCAN_VALU and for scenes without the operands, the all-VALU scan over the caller's order.  RTW_FLAG_GROUP_CULL is
    // accepted and runs the same scans: the words are the same by definition, and the cull layout has not been measured on primary rays.
    const int numerics = (p->flags & RTW_FLAG_NUMERICS_CONTRACT) ? rtw::NUM_CONTRACT : (p->flags & RTW_FLAG_NUMERICS_REFERENCE_FMA2) ? rtw::NUM_REFERENCE_FMA2 : rtw::NUM_REFERENCE;
    const bool mfma = scene->mf_ops != nullptr && !(p->flags & RTW_FLAG_SCAN_VALU);
    const size_t geom_bytes = (size_t)rtw::scene_geom_alloc(scene->n, scene->n_pad) * sizeof(V4);
    const bool lds_scene = geom_bytes <= RTW_LDS_SCENE_MAX_BYTES;             // (decided by the caller-order bytes, like the trace kernel's instance)
    rtw::DevScene<T> S = dev_scene_of<T>(scene);
    size_t scene_bytes = geom_bytes;
    if (mfma) {
        if (!scene->p_mf_ops || !scene->p_orig) return fail(-9, "internal: the scene has no arrays in the plain scan's order");
        S = dev_scene_plain_of<T>(scene);
        const size_t na = (size_t)rtw::scene_geom_alloc(S.n, S.n_pad);
        scene_bytes = na * sizeof(V4) + ((na * sizeof(unsigned short) + 15) / 16) * 16;
    }
    S.numerics = numerics;
    const size_t lds_bytes = rtw::feat_fixed_lds_bytes<T>() + (lds_scene ? scene_bytes : 0);
    typedef void (*kern_t)(rtw::FeatParams, rtw::Camera<T>, rtw::DevScene<T>, T *, rtw::DevCounters *);
    kern_t kern;
    if (mfma) kern = lds_scene ? (kern_t)rtw::features_kernel<T, true, true> : (kern_t)rtw::features_kernel<T, true, false>;
    else kern = lds_scene ? (kern_t)rtw::features_kernel<T, false, true> : (kern_t)rtw::features_kernel<T, false, false>;
    // the default numerics mode of the headline variant (scene in LDS, matrix pipe): the mode fixed at compile time
    if (mfma && lds_scene && numerics == rtw::NUM_REFERENCE) kern = (kern_t)rtw::features_kernel<T, true, true, rtw::NUM_REFERENCE>;
    const unsigned grid = (K.n_tiles + RTW_FEATURE_WAVES - 1u) / RTW_FEATURE_WAVES;
    // (test aid: which instance the rules above picked, in the form of the trace kernel's line -- rtw_launch.hip; the grid is one workgroup
    //  per RTW_FEATURE_WAVES tiles, no occupancy question is asked: blocks_per_cu=0)
    static const bool debug = aid_env("RTW_DEBUG") != nullptr;
    if (debug)
        fprintf(stderr, "[rtw debug] features instance: %s lds_scene=%d cull=0 mfma=%d fixed=%d batch=0 accum=0 adapt=0 lds_bytes=%zu blocks_per_cu=0\n", sizeof(T) == 8 ? "f64" : "f32",
                (int)lds_scene, (int)mfma, (int)(mfma && lds_scene && numerics == rtw::NUM_REFERENCE), lds_bytes);

    RenderRec *rec;
    if (int rc = acquire_rec(ctx.get(), &rec)) return rc;
    *rec_out = rec;
    rec->n_spheres = scene->n; rec->n_chunks = nch; rec->grid = (int)grid; rec->block = 64 * RTW_FEATURE_WAVES;
    rec->ctr_bytes = offsetof(rtw::DevCounters, t_first);
    HIP_TRY(hipMemsetAsync(rec->ctr, 0, rec->fresh ? sizeof(rtw::DevCounters) : rec->ctr_bytes, stream));
    rec->fresh = false;
    HIP_TRY(hipEventRecord(rec->ev0, stream));
    (void)hipGetLastError();           // (hipEventQuery's hipErrorNotReady in acquire_rec must not be mistaken for a launch failure)
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * RTW_FEATURE_WAVES), lds_bytes, stream, K, C, S, (T *)d_out, rec->ctr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(rec->ev1, stream));
    HIP_TRY(hipMemcpyAsync(rec->h_ctr, rec->ctr, rec->ctr_bytes, hipMemcpyDeviceToHost, stream));     // (into pinned memory: truly asynchronous)
    HIP_TRY(hipEventRecord(rec->ev2, stream));
    rec->used = true; rec->done = false;
    return 0;
}

int launch_features_f32(rtw_scene_handle scene, const rtw_camera_f32 *cam, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, void *d_out, hipStream_t stream,
                        RenderRec **rec_out, CtxPtr *ctx_out) {
    return launch_features<float>(scene, cam, p, chunk_begin, chunk_count, d_out, stream, rec_out, ctx_out);
}
int launch_features_f64(rtw_scene_handle scene, const rtw_camera_f64 *cam, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, void *d_out, hipStream_t stream,
                        RenderRec **rec_out, CtxPtr *ctx_out) {
    return launch_features<double>(scene, cam, p, chunk_begin, chunk_count, d_out, stream, rec_out, ctx_out);
}

template <typename CamT>
int features_device(rtw_scene_handle scene, const CamT *cam, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, void *d_out, void *stream_v) {
    if (!p) return fail(-1, "null params");
    if (!scene || !cam || !d_out) return fail(-1, "null argument");
    int nch, cs;
    if (int rc = validate_features(p, chunk_begin, chunk_count, &nch, &cs)) return rc;
    if (((uintptr_t)d_out & 15u) != 0) return fail(-2, "the feature buffer must be 16-byte aligned");
    DeviceGuard guard;
    RenderRec *rec = nullptr;
    CtxPtr ctx;
    release_last();
    int rc = launch_features_t(scene, cam, p, chunk_begin, chunk_count, d_out, (hipStream_t)stream_v, &rec, &ctx);
    if (rec) { g_last.recs.push_back(rec); g_last.ctxs.push_back(ctx); }       // (also on a late error: released by the next call)
    return rc;
}

}  // namespace rtwh

using namespace rtwh;

extern "C" {

int rtw_render_features_device_f32(rtw_scene_handle s, const rtw_camera_f32 *c, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, void *d_out, void *stream) {
    return features_device(s, c, p, chunk_begin, chunk_count, d_out, stream);
}
int rtw_render_features_device_f64(rtw_scene_handle s, const rtw_camera_f64 *c, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, void *d_out, void *stream) {
    return features_device(s, c, p, chunk_begin, chunk_count, d_out, stream);
}
int rtw_render_features_f32(const rtw_scene_f32 *s, const rtw_camera_f32 *c, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, float *out) {
    return render_host_features_f32(s, c, p, chunk_begin, chunk_count, out);
}
int rtw_render_features_f64(const rtw_scene_f64 *s, const rtw_camera_f64 *c, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, double *out) {
    return render_host_features_f64(s, c, p, chunk_begin, chunk_count, out);
}

}  // extern "C"
