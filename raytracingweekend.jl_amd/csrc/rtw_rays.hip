// rtw_rays.hip -- ray queries (include/rtw_hip.h rtw_cast_rays_*): the checks that need no device, ONE launch of the ray kernel (rtw_rays.hpp)
// per call -- its instance and its persistent grid; numerics mode and scene view (rtw_scene_view.hpp) and the record sequence (rtw_host.hpp
// begin_record / run_record) are the ones launch_features (rtw_features.hip) uses --, and the device-resident entry points.
// (The host-buffer entry points live with the other cached-context paths in rtw_render_host.hip.)
#include "rtw_scene_view.hpp"
#include "rtw_rays.hpp"

namespace rtwh {

// Everything about a ray query that is decided without a device and without a pointer: the parameters and the count (n == 0 is legal).
int validate_rays(const rtw_rays_params *p, int64_t n) {
    if (!p) return fail(-1, "null params");
    if (n < 0) return fail(-2, "negative ray count %lld", (long long)n);
    if (p->flags & ~(RTW_FLAG_GROUP_CULL | RTW_FLAG_SCAN_VALU | RTW_FLAG_NUMERICS_CONTRACT | RTW_FLAG_NUMERICS_REFERENCE_FMA2))
        return fail(-2, "a ray query takes the scan-mode and numerics flags only (flags 0x%x)", p->flags);
    { const int nm = p->flags & (RTW_FLAG_NUMERICS_CONTRACT | RTW_FLAG_NUMERICS_REFERENCE_FMA2);
      if (nm & (nm - 1)) return fail(-2, "the RTW_FLAG_NUMERICS_* bits exclude each other (flags 0x%x)", p->flags); }
    if (p->reserved != 0) return fail(-2, "rtw_rays_params.reserved must be 0");
    if (p->device < -1) return fail(-2, "bad device %d", p->device);
    if (p->max_workgroups < 0) return fail(-2, "max_workgroups must be 0 (automatic) or >= 1 (got %d)", p->max_workgroups);
    if (!std::isfinite(p->tmin) || p->tmin < 0) return fail(-2, "tmin must be finite and >= 0 (got %g)", p->tmin);
    if (n >= (1ll << 31)) return fail(-5, "too many rays for one call: %lld", (long long)n);
    return 0;
}

template <typename T>
static const void *rays_instance(bool mfma, bool lds_scene) {
    if (mfma) return lds_scene ? (const void *)rtw::cast_rays_kernel<T, true, true> : (const void *)rtw::cast_rays_kernel<T, true, false>;
    return lds_scene ? (const void *)rtw::cast_rays_kernel<T, false, true> : (const void *)rtw::cast_rays_kernel<T, false, false>;
}

// Enqueue the ray kernel for the n >= 1 rays at d_rays (validate_rays has accepted p and n) on `stream`; `rec_out` receives the counters
// and the kernel's events like a render's.  d_rec null: no records.
template <typename T>
int launch_rays(rtw_scene_handle scene, const void *d_rays, int64_t n, const rtw_rays_params *p, void *d_idx, void *d_rec, hipStream_t stream, RenderRec **rec_out, CtxPtr *ctx_out) {
    if (!scene || !d_rays || !p || !d_idx) return fail(-1, "null argument");
    if (((uintptr_t)d_rays & 15u) != 0 || ((uintptr_t)d_rec & 15u) != 0) return fail(-2, "the rays and the records must be 16-byte aligned");
    if (((uintptr_t)d_idx & 3u) != 0) return fail(-2, "the indices must be 4-byte aligned");
    if (scene->is_f64 != (sizeof(T) == 8)) return fail(-4, "scene handle precision does not match the call");
    if (p->device >= 0 && p->device != scene->device)
        return fail(-4, "params.device %d != scene device %d", p->device, scene->device);
    CtxPtr ctx;
    if (int rc = get_ctx(scene->device, &ctx)) return rc;
    *ctx_out = ctx;
    HIP_TRY(hipSetDevice(scene->device));

    rtw::RayParams K;
    K.n = (unsigned)n;
    K.n_batches = (unsigned)((n + 63) / 64);
    const T tmin = (T)p->tmin;
    // the scans of the feature pass (rtw_features.hip): pass 1 on the matrix pipe over the plain scan's own sphere order, or, under
    // RTW_FLAG_SCAN_VALU and for scenes without the operands, the all-VALU scan over the caller's order.  RTW_FLAG_GROUP_CULL is accepted and
    // runs the same scans: the words are the same by definition, and the cull layout has not been measured on caller rays.
    const int numerics = numerics_of(p->flags);
    const bool mfma = scene->mf_ops != nullptr && !(p->flags & RTW_FLAG_SCAN_VALU);
    PlainView<T> V;
    if (int rc = plain_scene_view<T>(scene, mfma, numerics, &V)) return rc;
    const size_t lds_bytes = rtw::rays_fixed_lds_bytes() + (V.lds_scene ? V.scene_bytes : 0);
    const void *kern = rays_instance<T>(mfma, V.lds_scene);
    // the persistent grid: what is resident at the kernel's occupancy for the LDS really requested (asked of the runtime once per context)
    int blocks_per_cu = 0;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        for (auto &o : ctx->occupancy) if (o.first.first == kern && o.first.second == lds_bytes) blocks_per_cu = o.second;
        if (blocks_per_cu < 1) {
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, kern, 64 * RTW_RAYS_WAVES, lds_bytes));
            ctx->occupancy.push_back({{kern, lds_bytes}, blocks_per_cu});
        }
    }
    if (blocks_per_cu < 1) blocks_per_cu = 1;
    const int grid = rays_grid(n, ctx->num_cus, blocks_per_cu, p->max_workgroups);
    // (test aid: which instance the rules above picked, in the form of the feature kernel's line)
    static const bool debug = aid_env("RTW_DEBUG") != nullptr;
    if (debug)
        fprintf(stderr, "[rtw debug] rays instance: %s lds_scene=%d cull=0 mfma=%d records=%d lds_bytes=%zu blocks_per_cu=%d grid=%d\n", sizeof(T) == 8 ? "f64" : "f32",
                (int)V.lds_scene, (int)mfma, (int)(d_rec != nullptr), lds_bytes, blocks_per_cu, grid);

    if (int rc = begin_record(ctx.get(), scene, 1, grid, 64 * RTW_RAYS_WAVES, offsetof(rtw::DevCounters, t_first), stream, rec_out)) return rc;
    void *args[] = {&K, (void *)&tmin, &V.scene, &d_rays, &d_idx, &d_rec, &(*rec_out)->ctr};
    return run_record(*rec_out, stream, [&] { (void)hipLaunchKernel(kern, dim3((unsigned)grid), dim3(64 * RTW_RAYS_WAVES), args, lds_bytes, stream); });
}

// The device-resident entry point: nulls, the parameters, the pointers' alignment, then the handle and what needs it.
template <typename T>
static int rays_device(rtw_scene_handle scene, const void *d_rays, int64_t n, const rtw_rays_params *p, void *d_idx, void *d_rec, void *stream_v) {
    if (!p) return fail(-1, "null params");
    if (!scene || !d_rays || !d_idx) return fail(-1, "null argument");
    if (int rc = validate_rays(p, n)) return rc;
    if (((uintptr_t)d_rays & 15u) != 0 || ((uintptr_t)d_rec & 15u) != 0) return fail(-2, "the rays and the records must be 16-byte aligned");
    if (((uintptr_t)d_idx & 3u) != 0) return fail(-2, "the indices must be 4-byte aligned");
    if (scene->is_f64 != (sizeof(T) == 8)) return fail(-4, "scene handle precision does not match the call");
    if (p->device >= 0 && p->device != scene->device) return fail(-4, "params.device %d != scene device %d", p->device, scene->device);
    if (n == 0) return 0;               // nothing enqueued; this thread's last render is left alone
    DeviceGuard guard;
    RenderRec *rec = nullptr;
    CtxPtr ctx;
    release_last();
    int rc = launch_rays<T>(scene, d_rays, n, p, d_idx, d_rec, (hipStream_t)stream_v, &rec, &ctx);
    hold_last(rec, ctx);               // (also on a late error: released by the next call)
    return rc;
}

template int launch_rays<float>(rtw_scene_handle, const void *, int64_t, const rtw_rays_params *, void *, void *, hipStream_t, RenderRec **, CtxPtr *);
template int launch_rays<double>(rtw_scene_handle, const void *, int64_t, const rtw_rays_params *, void *, void *, hipStream_t, RenderRec **, CtxPtr *);

}  // namespace rtwh

using namespace rtwh;

extern "C" {

int rtw_cast_rays_device_f32(rtw_scene_handle scene, const void *d_rays, int64_t n, const rtw_rays_params *p, void *d_idx, void *d_rec, void *hip_stream) {
    return rays_device<float>(scene, d_rays, n, p, d_idx, d_rec, hip_stream);
}
int rtw_cast_rays_device_f64(rtw_scene_handle scene, const void *d_rays, int64_t n, const rtw_rays_params *p, void *d_idx, void *d_rec, void *hip_stream) {
    return rays_device<double>(scene, d_rays, n, p, d_idx, d_rec, hip_stream);
}

}  // extern "C"
