// rtw_host_ctx.hpp -- what the two units of host-buffer entry points share (rtw_render_host.hip: the calls that render; rtw_stage_host.hip: the
// pure stages): the lease of a cached per-device context, its buffers, the ONE one-device path (stage_one_device; render_one_device: the same
// with a scene and a record) and the stages' regions inside a context's device buffer.
#pragma once
#include "rtw_host.hpp"

namespace rtwh {

static_assert(LAYOUT_FEATURE_CHANNELS == RTW_FEATURE_CHANNELS, "rtw_layout.hpp counts the feature channels itself");

// ---- the context pool (rtw_render_host.hip) --------------------------------------------------------------------------
// the caller holds a HostCtx exclusively between acquire and release
struct HostLease {
    CtxPtr ctx;
    HostCtx *hc = nullptr;
    bool pooled = false;
    ~HostLease() {
        if (!hc) return;
        if (pooled) { std::lock_guard<std::mutex> lk(ctx->mu); hc->busy = false; }
        else delete hc;                               // more concurrent host renders than pool entries: a temporary
    }
};
// `key` empty: no scene wanted -- the idle entry used last, whatever it holds; else the entry that holds this scene, or one to upload it into
int acquire_host(int device, const std::vector<unsigned char> &key, HostLease *out);
int ensure_dev(void **p, size_t *cap, size_t bytes);
int ensure_stage(HostCtx *hc, size_t bytes);          // the context's pinned staging buffer holds at least `bytes`
// Device image -> the caller's (pageable) buffer: ONE hipMemcpyAsync on the context's stream, then the stream drains.
int copy_out(HostCtx *hc, const void *d_src, void *out, size_t bytes);

template <typename SceneT>
void scene_key_of(const SceneT *s, bool f64, std::vector<unsigned char> &key) {
    using T = typename std::remove_cv<typename std::remove_pointer<decltype(s->cx)>::type>::type;
    const size_t n = (size_t)(s->n > 0 ? s->n : 0);
    key.clear();
    key.reserve(16 + n * (8 * sizeof(T) + sizeof(int32_t)));
    auto put = [&](const void *p, size_t b) { const unsigned char *q = (const unsigned char *)p; key.insert(key.end(), q, q + b); };
    const int32_t head[2] = {f64 ? 1 : 0, s->n};
    put(head, sizeof head);
    if (n == 0) return;
    const T *arrs[8] = {s->cx, s->cy, s->cz, s->r, s->ar, s->ag, s->ab, s->param};
    for (const T *a : arrs) put(a, n * sizeof(T));
    put(s->kind, n * sizeof(int32_t));
}

// `keep` non-null (render_host_animation): the upload this one replaces may still be read by launches on the stream -- it is handed over, not freed
template <typename T, typename SceneT>
int ensure_scene(HostCtx *hc, const SceneT *scene, const std::vector<unsigned char> &key, std::vector<ScenePtr> *keep = nullptr) {
    if (hc->scene && hc->scene_key == key) return 0;
    if (hc->scene && keep) { keep->emplace_back(hc->scene); hc->scene = nullptr; hc->scene_key.clear(); }
    if (hc->scene) { rtw_scene_free(hc->scene); hc->scene = nullptr; hc->scene_key.clear(); }
    if (int rc = upload_scene<T>(scene, hc->device, &hc->scene)) return rc;
    hc->scene_key = key;
    return 0;
}

// The one-device host path of a stage on host buffers, after the entry point's own validation: the caller's current device restored on
// return, a leased context of `device` (negative: the current device) with `dev_bytes` bytes of device buffer (0: none asked for), the
// `ups` as H2D copies in their order (`up_what` names them in the error text), launch(hc, base) -- it enqueues the stage on hc->stream
// over the regions of base = hc->d_img --, the `extras` as D2H copies in their order (`down_what`), the D2H of `result` last.  A copy whose
// host pointer is null or that is empty is skipped.  `scene` nullptr (every stage but the motion pass): the idle entry used last, the
// scene it may hold left alone; a scene: the entry that holds it, uploaded when it does not.  There is no record: this thread's last
// render (rtw_stats) is not touched.  The stream has drained when it returns, on success and on an error.
struct Upload { size_t off; const void *src; size_t bytes; };
struct Download { size_t off; void *dst; size_t bytes; };
template <typename T, typename SceneP, typename Launch>
int stage_one_device(int device, SceneP scene, size_t dev_bytes, const char *up_what, std::initializer_list<Upload> ups, Launch launch, Download result,
                     std::initializer_list<Download> extras = {}, const char *down_what = "") {
    constexpr bool with_scene = !std::is_null_pointer<SceneP>::value;
    DeviceGuard guard;
    std::vector<unsigned char> key;
    if constexpr (with_scene) scene_key_of(scene, sizeof(T) == 8, key);
    HostLease L;
    if (int rc = acquire_host(device, key, &L)) return rc;
    HostCtx *hc = L.hc;
    if constexpr (with_scene) { if (int rc = ensure_scene<T>(hc, scene, key)) return rc; }
    if (dev_bytes) if (int rc = ensure_dev(&hc->d_img, &hc->d_cap, dev_bytes)) return rc;
    char *base = (char *)hc->d_img;
    hipError_t e = hipSuccess;
    for (const Upload &u : ups)
        if (e == hipSuccess && u.src && u.bytes) e = hipMemcpyAsync(base + u.off, u.src, u.bytes, hipMemcpyHostToDevice, hc->stream);
    int rc = e == hipSuccess ? 0 : fail((int)e, "upload of %s failed: %s", up_what, hipGetErrorString(e));
    if (!rc) rc = launch(hc, base);
    for (const Download &d : extras)
        if (!rc && d.dst && d.bytes) if ((e = hipMemcpyAsync(d.dst, base + d.off, d.bytes, hipMemcpyDeviceToHost, hc->stream)) != hipSuccess)
            rc = fail((int)e, "download of %s failed: %s", down_what, hipGetErrorString(e));
    if (!rc) rc = copy_out(hc, base + result.off, result.dst, result.bytes);
    if (rc) (void)hipStreamSynchronize(hc->stream);           // nothing of this call may still be in flight when the lease ends
    return rc;
}

// The one-device host path of every host-buffer entry point that renders: the stage path above with the scene and no H2D -- ONE launch
// sequence: launch(hc, q, &rec, &ctx) enqueues it on hc->stream into hc->d_img, q: the caller's params bound to the lease's device --, ONE
// D2H of the `out_bytes` bytes at `out_off` into `out`, then the counters of `rec` into this thread's last render.
// (dev_bytes == 0, render_host's alone: a compact shard that owns no tile -- nothing is launched)
template <typename T, typename SceneT, typename Launch>
int render_one_device(int device, const SceneT *scene, const rtw_params *p, size_t dev_bytes, size_t out_off, size_t out_bytes, T *out, Launch launch) {
    if (s_has_bad_scene(scene)) return fail(-1, "null scene array");
    rtw_params q = *p;
    q.n_devices = 0; q.device_ids = nullptr;
    RenderRec *rec = nullptr;
    CtxPtr rctx;
    int rc = stage_one_device<T>(device, scene, dev_bytes, "", {}, [&](HostCtx *hc, char *) {
        q.device = hc->device;
        return dev_bytes ? launch(hc, q, &rec, &rctx) : 0;
    }, {out_off, out, dev_bytes ? out_bytes : 0});
    if (!rc && dev_bytes) rc = resolve_rec(rec, &g_last.agg);
    if (!rc && dev_bytes) g_last.per_device.emplace_back(q.device, g_last.agg.kernel_ms);
    if (rec) release_rec(rctx, rec, rc == 0);
    g_last.resolved = rc == 0;
    return rc;
}

// ---- the stages' regions inside a context's device buffer (rtw_layout.hpp) with the sizes the library itself reports ---------------------
template <typename T> struct DenoiseRegions : DenoiseLayout {
    DenoiseRegions(int32_t width, int32_t height, int32_t n_views) : DenoiseLayout(sizeof(T), width, height, n_views, (size_t)rtw_denoise_work_bytes(width, height, (int32_t)sizeof(T))) {}
    // the filter over the regions of `base`, on `stream`
    int launch(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views, char *base, hipStream_t stream, const void *d_noise = nullptr) const {
        return launch_denoise<T>(d, width, height, n_views, base, base + off_feat, base + off_out, base + off_work, stream, d_noise);
    }
};

template <typename T> struct UpsampleRegions : UpsampleLayout {
    UpsampleRegions(int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, int32_t n_views)
        : UpsampleLayout(sizeof(T), lo_width, lo_height, width, height, n_views, (size_t)rtw_upsample_work_bytes(lo_width, lo_height, (int32_t)sizeof(T))) {}
    // the upsampler over the regions of `base`, on `stream`
    int launch(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, int32_t n_views, char *base, hipStream_t stream) const {
        return launch_upsample<T>(u, lo_width, lo_height, width, height, n_views, base, base + off_flo, base + off_fhi, base + off_out, base + off_work, stream);
    }
};

template <typename T> struct TemporalRegions : TemporalLayout {
    TemporalRegions(int32_t width, int32_t height, size_t frames, bool filter, size_t paths = 1)
        : TemporalLayout(sizeof(T), width, height, frames, filter, paths, (size_t)rtw_temporal_state_bytes(width, height, (int32_t)sizeof(T)),
                         (size_t)rtw_denoise_work_bytes(width, height, (int32_t)sizeof(T))) {}
};

template <typename T> struct MomentRegions : MomentLayout {
    MomentRegions(int32_t width, int32_t height, size_t frames, bool filter, size_t paths = 1, bool moments = true)
        : MomentLayout(sizeof(T), width, height, frames, filter, paths, moments, (size_t)rtw_temporal_state_bytes(width, height, (int32_t)sizeof(T)),
                       (size_t)rtw_denoise_work_bytes(width, height, (int32_t)sizeof(T)), (size_t)rtw_history_moment_bytes(width, height, (int32_t)sizeof(T))) {}
};

}  // namespace rtwh
