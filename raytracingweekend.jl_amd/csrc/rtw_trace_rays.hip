// rtw_trace_rays.hip -- radiance queries (include/rtw_hip.h rtw_trace_rays_*): the checks that need no device, ONE launch of the radiance
// kernel (rtw_trace_rays.hpp) per call -- its instance table and its grid from the occupancy answer asked once per context; numerics mode,
// scene view and record sequence are the ones launch_rays (rtw_rays.hip) uses --, and the device-resident entry points.
// (The host-buffer entry points live with the other cached-context paths in rtw_render_host.hip.)
#include "rtw_scene_view.hpp"
#include "rtw_trace_rays.hpp"

namespace rtwh {

// Everything about a radiance query that is decided without a device and without a pointer: the parameters and the count (n == 0 is legal).
int validate_trace_rays(const rtw_trace_params *p, int64_t n) {
    if (!p) return fail(-1, "null params");
    if (n < 0) return fail(-2, "negative ray count %lld", (long long)n);
    if (p->flags & ~(RTW_FLAG_GROUP_CULL | RTW_FLAG_SCAN_VALU | RTW_FLAG_NUMERICS_CONTRACT | RTW_FLAG_NUMERICS_REFERENCE_FMA2))
        return fail(-2, "a radiance query takes the scan-mode and numerics flags only (flags 0x%x)", p->flags);
    { const int nm = p->flags & (RTW_FLAG_NUMERICS_CONTRACT | RTW_FLAG_NUMERICS_REFERENCE_FMA2);
      if (nm & (nm - 1)) return fail(-2, "the RTW_FLAG_NUMERICS_* bits exclude each other (flags 0x%x)", p->flags); }
    if (p->reserved != 0) return fail(-2, "rtw_trace_params.reserved must be 0");
    if (p->device < -1) return fail(-2, "bad device %d", p->device);
    if (p->max_workgroups < 0) return fail(-2, "max_workgroups must be 0 (automatic) or >= 1 (got %d)", p->max_workgroups);
    if (p->spp < 1) return fail(-2, "spp must be >= 1 (got %d)", p->spp);
    if (p->max_depth < 0 || p->max_depth >= (1 << 22)) return fail(-2, "max_depth must be in [0, 2^22)");
    if (n >= (1ll << 31)) return fail(-5, "too many rays for one call: %lld", (long long)n);
    if (u64_range_wraps(p->first_stream, (uint64_t)n)) return fail(-2, "first_stream + n leaves the 64-bit range");
    if (u64_range_wraps(p->first_sample, (uint64_t)p->spp)) return fail(-2, "first_sample + spp leaves the 64-bit range");
    return 0;
}

// the checks of the device pointers and of the handle, in the order of the header's list
static int check_trace_rays_device(rtw_scene_handle scene, const void *d_rays, const rtw_trace_params *p, const void *d_out, bool is_f64) {
    if (((uintptr_t)d_rays & 15u) != 0) return fail(-2, "the rays must be 16-byte aligned");
    if (((uintptr_t)d_out & 7u) != 0) return fail(-2, "the results must be 8-byte aligned");
    if (scene->is_f64 != is_f64) return fail(-4, "scene handle precision does not match the call");
    if (p->device >= 0 && p->device != scene->device) return fail(-4, "params.device %d != scene device %d", p->device, scene->device);
    return 0;
}

template <typename T>
static const void *trace_rays_instance(bool mfma, bool lds_scene) {
    if (mfma) return lds_scene ? (const void *)rtw::trace_rays_kernel<T, true, true> : (const void *)rtw::trace_rays_kernel<T, true, false>;
    return lds_scene ? (const void *)rtw::trace_rays_kernel<T, false, true> : (const void *)rtw::trace_rays_kernel<T, false, false>;
}

// Enqueue the radiance kernel for the n >= 1 rays at d_rays (validate_trace_rays has accepted p and n) on `stream`; `rec_out` receives the
// counters and the kernel's events like a render's.
template <typename T>
int launch_trace_rays(rtw_scene_handle scene, const void *d_rays, int64_t n, const rtw_trace_params *p, void *d_out, hipStream_t stream, RenderRec **rec_out, CtxPtr *ctx_out) {
    if (!scene || !d_rays || !p || !d_out) return fail(-1, "null argument");
    if (int rc = check_trace_rays_device(scene, d_rays, p, d_out, sizeof(T) == 8)) return rc;
    CtxPtr ctx;
    if (int rc = get_ctx(scene->device, &ctx)) return rc;
    *ctx_out = ctx;
    HIP_TRY(hipSetDevice(scene->device));

    rtw::TraceRaysParams K;
    K.n = (unsigned)n;
    K.n_batches = trace_rays_batches(n);
    K.spp = p->spp; K.max_depth = p->max_depth;
    K.seed = p->seed; K.first_stream = p->first_stream; K.first_sample = p->first_sample;
    // the scans of the ray queries (rtw_rays.hip): the matrix pipe over the plain scan's own sphere order, or, under RTW_FLAG_SCAN_VALU and for
    // scenes without the operands, the all-VALU scan over the caller's order.  RTW_FLAG_GROUP_CULL is accepted and runs the same scans.
    const int numerics = numerics_of(p->flags);
    const bool mfma = scene->mf_ops != nullptr && !(p->flags & RTW_FLAG_SCAN_VALU);
    PlainView<T> V;
    if (int rc = plain_scene_view<T>(scene, mfma, numerics, &V)) return rc;
    const size_t lds_bytes = rtw::rays_fixed_lds_bytes() + (V.lds_scene ? V.scene_bytes : 0);
    const void *kern = trace_rays_instance<T>(mfma, V.lds_scene);
    // the grid: what is resident at the kernel's occupancy for the LDS really requested (asked of the runtime once per context)
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
    const int grid = trace_rays_grid(n, ctx->num_cus, blocks_per_cu, p->max_workgroups);
    // (test aid: which instance the rules above picked, in the form of the ray kernel's line)
    static const bool debug = aid_env("RTW_DEBUG") != nullptr;
    if (debug)
        fprintf(stderr, "[rtw debug] trace_rays instance: %s lds_scene=%d cull=0 mfma=%d spp=%d lds_bytes=%zu blocks_per_cu=%d grid=%d\n", sizeof(T) == 8 ? "f64" : "f32",
                (int)V.lds_scene, (int)mfma, p->spp, lds_bytes, blocks_per_cu, grid);

    // (the record's counters are zeroed on `stream` up to t_first: the kernel's batch counter, DevCounters::next_job[0], among them)
    if (int rc = begin_record(ctx.get(), scene, 1, grid, 64 * RTW_RAYS_WAVES, offsetof(rtw::DevCounters, t_first), stream, rec_out)) return rc;
    void *args[] = {&K, &V.scene, &d_rays, &d_out, &(*rec_out)->ctr};
    return run_record(*rec_out, stream, [&] { (void)hipLaunchKernel(kern, dim3((unsigned)grid), dim3(64 * RTW_RAYS_WAVES), args, lds_bytes, stream); });
}

// The device-resident entry point: nulls, the parameters, the pointers' alignment, then the handle and what needs it.
template <typename T>
static int trace_rays_device(rtw_scene_handle scene, const void *d_rays, int64_t n, const rtw_trace_params *p, void *d_out, void *stream_v) {
    if (!p) return fail(-1, "null params");
    if (!scene || !d_rays || !d_out) return fail(-1, "null argument");
    if (int rc = validate_trace_rays(p, n)) return rc;
    if (int rc = check_trace_rays_device(scene, d_rays, p, d_out, sizeof(T) == 8)) return rc;
    if (n == 0) return 0;               // nothing enqueued; this thread's last render is left alone
    DeviceGuard guard;
    RenderRec *rec = nullptr;
    CtxPtr ctx;
    release_last();
    int rc = launch_trace_rays<T>(scene, d_rays, n, p, d_out, (hipStream_t)stream_v, &rec, &ctx);
    hold_last(rec, ctx);               // (also on a late error: released by the next call)
    return rc;
}

template int launch_trace_rays<float>(rtw_scene_handle, const void *, int64_t, const rtw_trace_params *, void *, hipStream_t, RenderRec **, CtxPtr *);
template int launch_trace_rays<double>(rtw_scene_handle, const void *, int64_t, const rtw_trace_params *, void *, hipStream_t, RenderRec **, CtxPtr *);

}  // namespace rtwh

using namespace rtwh;

extern "C" {

int rtw_trace_rays_device_f32(rtw_scene_handle scene, const void *d_rays, int64_t n, const rtw_trace_params *p, void *d_out, void *hip_stream) {
    return trace_rays_device<float>(scene, d_rays, n, p, d_out, hip_stream);
}
int rtw_trace_rays_device_f64(rtw_scene_handle scene, const void *d_rays, int64_t n, const rtw_trace_params *p, void *d_out, void *hip_stream) {
    return trace_rays_device<double>(scene, d_rays, n, p, d_out, hip_stream);
}

}  // extern "C"
