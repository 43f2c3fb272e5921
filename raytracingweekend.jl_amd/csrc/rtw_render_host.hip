// rtw_render_host.hip -- the host-buffer entry points of the C ABI that render (rtw_render_f32/_f64 is what the Julia ccall binds; replaces src/render.jl:8-44):
// the pool of cached per-device contexts (uploaded scene, stream, device buffer), one device (rtw_host_ctx.hpp render_one_device: the path the plain, the batched, the
// feature, the render + filter, the render + upsample, the sequence and the render + present entry points share) or a device list (tiles dealt round-robin, shards gathered on the first device by peer
// copies or ONE RCCL reduce: rtw_multi.hip), one D2H of the result.  The single and the batched form of a call share one body (n_views == 0: single);
// the three render + lens calls (defocused, wide aperture, lens batch) share render_host_lens.
// (The pure stages on host buffers: rtw_stage_host.hip.)
#include "rtw_host_ctx.hpp"

namespace rtwh {

// ---- host-buffer path --------------------------------------------------------------------------------------------
HostCtx::~HostCtx() {
    if (device >= 0) HIP_IGNORE(hipSetDevice(device));
    if (scene) rtw_scene_free(scene);
    if (d_img) HIP_IGNORE(hipFree(d_img));
    if (d_aux) HIP_IGNORE(hipFree(d_aux));
    if (h_stage) HIP_IGNORE(hipHostFree(h_stage));
    if (done_ev) HIP_IGNORE(hipEventDestroy(done_ev));
    if (stream) HIP_IGNORE(hipStreamDestroy(stream));
}

int acquire_host(int device, const std::vector<unsigned char> &key, HostLease *out) {
    int dev;
    if (int rc = resolve_device(device, &dev)) return rc;
    CtxPtr ctx;
    if (int rc = get_ctx(dev, &ctx)) return rc;
    out->ctx = ctx;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        HostCtx *pick = nullptr;
        if (key.empty()) {                                                                             // no scene wanted (the denoiser): the idle entry used last, whatever it holds
            for (auto &h : ctx->host) if (!h->busy && (!pick || h->last_use > pick->last_use)) pick = h.get();
        } else {
            for (auto &h : ctx->host) if (!h->busy && h->scene_key == key) { pick = h.get(); break; }     // same scene: nothing to upload
        }
        size_t idle = 0;
        for (auto &h : ctx->host) if (!h->busy) ++idle;
        if (!pick && ctx->host.size() < RTW_HOST_CTX_POOL && idle < RTW_HOST_CTX_IDLE_KEEP) {
            // a scene this device has not seen (or whose entries are all busy): a NEW entry while the pool has room and fewer than
            // RTW_HOST_CTX_IDLE_KEEP idle entries exist -- a caller that alternates between two or three scenes keeps them all uploaded,
            // concurrent callers get an entry each, but an animation (a new scene every frame from one thread) recycles the least
            // recently used idle entry instead of building eight contexts of ~200 MB each
            ctx->host.emplace_back(new HostCtx());
            pick = ctx->host.back().get();
            pick->device = dev;
        }
        if (!pick)                                                                                  // pool full: the least recently used idle entry
            for (auto &h : ctx->host) if (!h->busy && (!pick || h->last_use < pick->last_use)) pick = h.get();
        if (pick) { pick->busy = true; pick->last_use = ++ctx->use_clock; out->hc = pick; out->pooled = true; }
    }
    if (!out->hc) { out->hc = new HostCtx(); out->hc->device = dev; out->pooled = false; }
    HostCtx *hc = out->hc;
    HIP_TRY(hipSetDevice(dev));
    if (!hc->stream) HIP_TRY(hipStreamCreateWithFlags(&hc->stream, hipStreamNonBlocking));
    if (!hc->done_ev) HIP_TRY(hipEventCreateWithFlags(&hc->done_ev, hipEventDisableTiming));
    return 0;
}

int ensure_dev(void **p, size_t *cap, size_t bytes) {
    if (*cap >= bytes && *p) return 0;
    if (*p) { HIP_IGNORE(hipFree(*p)); *p = nullptr; *cap = 0; }
    HIP_TRY(hipMalloc(p, bytes));
    *cap = bytes;
    return 0;
}

int ensure_stage(HostCtx *hc, size_t bytes) {
    if (hc->stage_cap >= bytes) return 0;
    if (hc->h_stage) { HIP_IGNORE(hipHostFree(hc->h_stage)); hc->h_stage = nullptr; hc->stage_cap = 0; }
    HIP_TRY(hipHostMalloc(&hc->h_stage, bytes, hipHostMallocDefault));
    hc->stage_cap = bytes;
    return 0;
}

// Device image -> the caller's (pageable) buffer: ONE hipMemcpyAsync on the context's stream.  Measured on the MI355X box
// (tools/ubench_d2h.hip, 24.9 MB): straight into pageable memory 0.45 ms -- as fast as into pinned memory -- against 1.28 ms
// through a pinned staging buffer + memcpy and 0.6 - 1.0 ms for chunked staging overlapped with 1 - 4 memcpy threads.
int copy_out(HostCtx *hc, const void *d_src, void *out, size_t bytes) {
    if (bytes == 0) return 0;
    HIP_TRY(hipMemcpyAsync(out, d_src, bytes, hipMemcpyDeviceToHost, hc->stream));
    HIP_TRY(hipStreamSynchronize(hc->stream));
    return 0;
}

// the record of a pass beside the render's own (a feature pass), handed back when the call returns: the stream has drained by then, either way
struct SideRec { RenderRec *rec = nullptr; CtxPtr ctx; ~SideRec() { if (rec) release_rec(ctx, rec, true); } };

template <typename T, typename SceneT, typename CamT>
int render_host(const SceneT *scene, const CamT *cam, const rtw_params *p, T *out) {
    if (!scene || !cam || !p || !out) return fail(-1, "null argument");
    int nch, cs;
    if (int rc = validate_params(p, &nch, &cs)) return rc;
    DeviceGuard guard;
    release_last();
    // the device list (n_devices / device_ids; Julia keyword devices=:all)
    std::vector<int> devs;
    if (p->n_devices == -1) {
        int n = 0;
        const hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess || n <= 0)
            return fail(e != hipSuccess ? (int)e : -21, "no HIP device available (%s); librtw_hip has no CPU fallback",
                        e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
        for (int d = 0; d < n; ++d) devs.push_back(d);
    } else if (p->n_devices > 1 || (p->n_devices == 1 && p->device_ids)) {
        if (!p->device_ids) return fail(-1, "n_devices = %d but device_ids is null", p->n_devices);
        devs.assign(p->device_ids, p->device_ids + p->n_devices);
    } else if (p->n_devices < -1) {
        return fail(-2, "bad n_devices %d", p->n_devices);
    }
    if (devs.size() <= 1 && !((p->flags & RTW_FLAG_RCCL_REDUCE) && devs.size() == 1)) {
        // ---- one device: render into the cached device image, one D2H ----
        const size_t bytes = ((p->flags & RTW_FLAG_COMPACT_TILES) ? (size_t)local_tiles(p) * 64 * 3 : (size_t)p->width * (size_t)p->height * 3) * sizeof(T);
        return render_one_device(devs.size() == 1 ? devs[0] : p->device, scene, p, bytes, 0, bytes, out, [&](HostCtx *hc, rtw_params &q, RenderRec **rec, CtxPtr *rctx) {
            q.flags &= ~RTW_FLAG_RCCL_REDUCE;              // (one device: nothing to reduce)
            return launch_render<T>(hc->scene, cam, 0, nullptr, &q, hc->d_img, hc->stream, rec, rctx);
        });
    }
    if (s_has_bad_scene(scene)) return fail(-1, "null scene array");
    std::vector<unsigned char> key;
    scene_key_of(scene, sizeof(T) == 8, key);

    // ---- several devices: shard r renders tiles t = r (mod N) on its own device and stream, then ONE of
    //   (default)             compact tile-major shards gathered in HBM of the first device -- peer copies over xGMI with peer access
    //                         enabled per pair (ensure_peer; host-staged fallback when the platform refuses it); a shard on the root
    //                         device renders straight into the gather buffer --, un-tiled there by one small kernel;
    //   RTW_FLAG_RCCL_REDUCE  zero-padded full frames summed onto the first device by ONE ncclReduce over xGMI (BASELINE configs[3]'s
    //                         "RCCL reduce of per-tile framebuffers": x + 0 == x, so the sum is the image bit for bit);
    //      and the frame crosses PCIe once ----
    if (p->shard_count != 1) return fail(-2, "n_devices > 1 cannot be combined with shard_index/shard_count");
    if (p->flags & RTW_FLAG_COMPACT_TILES) return fail(-2, "n_devices > 1 writes the full frame (RTW_FLAG_COMPACT_TILES is a per-shard layout)");
    const int N = (int)devs.size();
    const bool use_rccl = (p->flags & RTW_FLAG_RCCL_REDUCE) != 0;
    static const bool dbg_remote = aid_flag("RTW_DEBUG_REMOTE_SHARDS");
    // (RCCL: the communicator set of this device list, locked for this render until its streams have drained -- RcclSet, rtw_multi.hip)
    std::shared_ptr<RcclSet> rccl_set;
    std::unique_lock<std::mutex> rccl_use;
    std::vector<HostLease> L(N);
    for (int r = 0; r < N; ++r)
        if (int rc = acquire_host(devs[r], key, &L[r])) return fail(rc, "device %d (shard %d of %d): %s", devs[r], r, N, std::string(g_err).c_str());
    if (use_rccl) { if (int rc = rccl_acquire(devs, &rccl_set, &rccl_use)) return rc; }       // (after the devices are known to exist; a host context is never waited for, so the order cannot deadlock)
    {   // scene uploads of the devices that do not have it yet, in parallel (a cache miss on 8 devices is 8 x (kd split + a dozen copies))
        std::vector<int> up_rc(N, 0);
        std::vector<std::string> up_err(N);
        std::vector<std::thread> th;
        for (int r = 0; r < N; ++r) {
            if (L[r].hc->scene && L[r].hc->scene_key == key) continue;
            th.emplace_back([&, r] { up_rc[r] = ensure_scene<T>(L[r].hc, scene, key); if (up_rc[r]) up_err[r] = g_err; });
        }
        for (auto &t : th) t.join();
        for (int r = 0; r < N; ++r)
            if (up_rc[r]) return fail(up_rc[r], "device %d (shard %d of %d): %s", devs[r], r, N, up_err[r].c_str());
    }
    HostCtx *root = L[0].hc;
    rtw_params q0 = *p;
    q0.shard_index = 0; q0.shard_count = N;
    const long pad_tiles = local_tiles(&q0);                               // shard 0 owns the most tiles
    const size_t shard_bytes = (size_t)pad_tiles * 192 * sizeof(T), frame_bytes = (size_t)p->width * p->height * 3 * sizeof(T);
    HIP_TRY(hipSetDevice(root->device));
    if (!use_rccl) { if (int rc = ensure_dev(&root->d_aux, &root->aux_cap, shard_bytes * N)) return rc; }
    if (int rc = ensure_dev(&root->d_img, &root->d_cap, frame_bytes)) return rc;
    std::vector<RenderRec *> recs(N, nullptr);
    std::vector<CtxPtr> rctx(N);
    int rc = 0, gather_path = 0;
    for (int r = 0; r < N && !rc; ++r) {
        HostCtx *hc = L[r].hc;
        rtw_params q = *p;
        q.device = hc->device; q.shard_index = r; q.shard_count = N; q.n_devices = 0; q.device_ids = nullptr;
        q.flags &= ~RTW_FLAG_RCCL_REDUCE;
        const hipError_t e0 = hipSetDevice(hc->device);
        if (e0 != hipSuccess) { rc = fail((int)e0, "hipSetDevice(%d): %s", hc->device, hipGetErrorString(e0)); break; }
        if (use_rccl) {
            // this shard's tiles in the full-frame layout, zero elsewhere (launch_render clears the frame of a sharded render first)
            if ((rc = ensure_dev(&hc->d_img, &hc->d_cap, frame_bytes))) break;
            rc = launch_render<T>(hc->scene, cam, 0, nullptr, &q, hc->d_img, hc->stream, &recs[r], &rctx[r]);
            continue;
        }
        q.flags |= RTW_FLAG_COMPACT_TILES;
        const size_t my_bytes = (size_t)local_tiles(&q) * 192 * sizeof(T);
        char *slot = (char *)root->d_aux + (size_t)r * shard_bytes;
        if (my_bytes == 0) continue;
        const bool remote = hc->device != root->device || (dbg_remote && hc != root);
        void *d_out = slot;
        if (remote) {
            if ((rc = ensure_dev(&hc->d_img, &hc->d_cap, my_bytes))) break;        // (the shard buffer belongs to ITS device)
            d_out = hc->d_img;
        }
        if ((rc = launch_render<T>(hc->scene, cam, 0, nullptr, &q, d_out, hc->stream, &recs[r], &rctx[r]))) break;
        hipError_t e = hipSuccess;
        bool staged = false;
        if (remote) {
            bool direct = false;
            if ((rc = ensure_peer(L[r].ctx, hc->device, root->device, &direct))) break;
            e = hipSetDevice(hc->device);                 // (ensure_peer switches devices while it enables the access)
            if (e != hipSuccess) { rc = fail((int)e, "hipSetDevice(%d): %s", hc->device, hipGetErrorString(e)); break; }
            if (direct) {
                gather_path |= RTW_GATHER_PEER;
                e = hipSetDevice(hc->device);
                if (e == hipSuccess) e = hipMemcpyPeerAsync(slot, root->device, d_out, hc->device, my_bytes, hc->stream);
            } else {
                // the documented fallback: through this shard's pinned staging buffer
                gather_path |= RTW_GATHER_HOST_STAGED;
                staged = true;
                if ((rc = ensure_stage(hc, my_bytes))) { rc = fail(rc, "device %d (shard %d of %d): gather failed: %s", hc->device, r, N, std::string(g_err).c_str()); break; }
                e = hipMemcpyAsync(hc->h_stage, d_out, my_bytes, hipMemcpyDeviceToHost, hc->stream);
            }
        } else if (hc != root) {
            gather_path |= RTW_GATHER_SAME_DEVICE;
        }
        if (e == hipSuccess) e = hipEventRecord(hc->done_ev, hc->stream);
        if (e == hipSuccess && hc != root) {
            e = hipSetDevice(root->device);
            if (e == hipSuccess) e = hipStreamWaitEvent(root->stream, hc->done_ev, 0);
            if (e == hipSuccess && staged) e = hipMemcpyAsync(slot, hc->h_stage, my_bytes, hipMemcpyHostToDevice, root->stream);
        }
        if (e != hipSuccess) rc = fail((int)e, "device %d (shard %d of %d): gather failed: %s", hc->device, r, N, hipGetErrorString(e));
    }
    if (!rc && use_rccl) {
        gather_path |= RTW_GATHER_RCCL;
        std::vector<const void *> send(N);
        std::vector<hipStream_t> streams(N);
        for (int r = 0; r < N; ++r) { send[r] = L[r].hc->d_img; streams[r] = L[r].hc->stream; }
        rc = rccl_reduce_frames(*rccl_set, send, root->d_img, (size_t)p->width * p->height * 3, sizeof(T) == 8, streams);
        if (!rc) { const hipError_t e = hipSetDevice(root->device); if (e != hipSuccess) rc = fail((int)e, "hipSetDevice: %s", hipGetErrorString(e)); }
        if (!rc) rc = copy_out(root, root->d_img, out, frame_bytes);
    } else if (!rc) {
        const hipError_t e = hipSetDevice(root->device);
        const long n_tiles = (long)((p->height + 7) / 8) * ((p->width + 7) / 8);
        if (e != hipSuccess) rc = fail((int)e, "hipSetDevice(%d): %s", root->device, hipGetErrorString(e));
        if (!rc) rc = launch_untile(sizeof(T) == 8, root->d_aux, root->d_img, p->width, p->height, n_tiles, N, pad_tiles, root->stream);
        if (!rc) rc = copy_out(root, root->d_img, out, frame_bytes);
    }
    // every stream of this call drains before the leases end, also on an error
    for (int r = 0; r < N; ++r) { HIP_IGNORE(hipSetDevice(L[r].hc->device)); HIP_IGNORE(hipStreamSynchronize(L[r].hc->stream)); }
    if (rccl_use.owns_lock()) rccl_use.unlock();           // the communicators are free for the next render of this device list
    rtw_stats_t &a = g_last.agg;                       // sums over the devices; times: the maximum
    for (int r = 0; r < N; ++r) {
        if (!recs[r]) {                                   // a shard that owns no tile (a tiny frame on many devices): launched nothing --
            if (!rc) g_last.per_device.emplace_back(L[r].hc->device, 0.0);     // still one entry per shard, in shard order (include/rtw_hip.h)
            continue;
        }
        rtw_stats_t st;
        memset(&st, 0, sizeof st);
        if (!rc) rc = resolve_rec(recs[r], &st);
        release_rec(rctx[r], recs[r], rc == 0);
        if (!rc) g_last.per_device.emplace_back(recs[r]->device, st.kernel_ms);
        a.samples += st.samples; a.segments += st.segments; a.sphere_tests += st.sphere_tests;
        a.kernel_ms = std::max(a.kernel_ms, st.kernel_ms); a.total_ms = std::max(a.total_ms, st.total_ms);
        a.n_chunks = st.n_chunks; a.grid_blocks = std::max(a.grid_blocks, st.grid_blocks); a.block_threads = std::max(a.block_threads, st.block_threads);
    }
    a.gather_path = gather_path;
    g_last.resolved = rc == 0;
    return rc;
}

// N views of one scene (rtw_render_batch_f32/_f64): the one-device path above with a device image of N frames, ONE launch, ONE D2H.
template <typename T, typename SceneT, typename CamT>
int render_host_batch(const SceneT *scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, T *out) {
    if (int rc = validate_batch(cams, n_views, p, out)) return rc;
    if (!scene) return fail(-1, "null argument");
    DeviceGuard guard;
    release_last();
    const size_t bytes = (size_t)n_views * (size_t)p->width * (size_t)p->height * 3 * sizeof(T);
    return render_one_device(p->device, scene, p, bytes, 0, bytes, out, [&](HostCtx *hc, rtw_params &q, RenderRec **rec, CtxPtr *rctx) {
        return launch_render<T>(hc->scene, cams, n_views, seeds, &q, hc->d_img, hc->stream, rec, rctx);
    });
}

// In everything below n_views == 0 is the single-view entry point and n_views != 0 the batched one (rtw_host.hpp batch_views): each keeps its
// own validation, what follows it is shared.

// First-hit feature buffers (rtw_render_features_* / rtw_render_features_batch_*): the one-device path above with a device buffer of W x H x 8
// elements per view, ONE launch of the feature kernel (rtw_features.hip; a BATCH instance for a batch), ONE D2H.
template <typename T, typename SceneT, typename CamT>
int render_host_features(const SceneT *scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, T *out) {
    if (!p) return fail(-1, "null params");
    if (!scene || !cams || !out) return fail(-1, "null argument");
    int nch, cs;
    if (int rc = n_views ? validate_features_batch(cams, n_views, p, chunk_begin, chunk_count, out, &nch, &cs) : validate_features(p, chunk_begin, chunk_count, &nch, &cs)) return rc;
    DeviceGuard guard;
    release_last();
    const size_t bytes = (size_t)(n_views ? n_views : 1) * (size_t)p->width * (size_t)p->height * RTW_FEATURE_CHANNELS * sizeof(T);
    return render_one_device(p->device, scene, p, bytes, 0, bytes, out, [&](HostCtx *hc, rtw_params &q, RenderRec **rec, CtxPtr *rctx) {
        return launch_features<T>(hc->scene, cams, n_views, seeds, &q, chunk_begin, chunk_count, hc->d_img, hc->stream, rec, rctx);
    });
}

// The first-hit motion pass on host buffers (rtw_first_hit_motion_*): the stage path (stage_one_device) with the scene -- a leased context of
// the device with the scene uploaded (the cached one when its bytes are the same) and a device buffer that holds the motion plane and, behind
// it, the motion table (`table`: scene->n rows of 4 elements, or null: m = 0 -- an id buffer); at most one H2D, ONE launch, ONE D2H.  The pass
// has no record: this thread's last render (rtw_stats) is not touched.
template <typename T, typename SceneT, typename CamT>
int render_host_motion(const SceneT *scene, const CamT *cam, const rtw_params *p, const T *table, T *motion) {
    if (!p) return fail(-1, "null params");
    if (!scene || !cam || !motion) return fail(-1, "null argument");
    if (int rc = validate_motion(p, (int)sizeof(T))) return rc;
    if (scene->n < 0) return fail(-2, "negative sphere count");
    if (s_has_bad_scene(scene)) return fail(-1, "null scene array");
    const size_t mo_b = (size_t)p->width * (size_t)p->height * 4 * sizeof(T), tab_b = (size_t)scene->n * 4 * sizeof(T);
    DevLayout L{mo_b};
    const size_t off_tab = L.add(tab_b);
    if (int rc = check_alias({{"motion", motion, mo_b}}, {{"table", table, tab_b}}, "the table")) return rc;
    return stage_one_device<T>(p->device, scene, L.total, "the motion table", {{off_tab, table, tab_b}},
        [&](HostCtx *hc, char *base) {
            rtw_params q = *p;
            q.device = hc->device;
            return launch_motion<T>(hc->scene, cam, &q, table && tab_b ? base + off_tab : nullptr, base, hc->stream);
        },
        {0, motion, mo_b});
}

// Ray queries on host buffers (rtw_cast_rays_*): the stage path (stage_one_device) WITH the scene and a record, as render_one_device runs
// it -- a leased context of the device with the scene uploaded (the cached one when its bytes are the same) and a device buffer that holds
// the indices, the records and the rays (RaysLayout); ONE H2D of the rays, ONE launch, ONE D2H of the records where asked for and ONE of
// the indices, then the counters of the record into this thread's last render.
template <typename T, typename SceneT>
int cast_rays_host(const SceneT *scene, const T *rays, int64_t n, const rtw_rays_params *p, int32_t *idx, T *rec) {
    if (!p) return fail(-1, "null params");
    if (!scene || !rays || !idx) return fail(-1, "null argument");
    if (int rc = validate_rays(p, n)) return rc;
    if (scene->n < 0) return fail(-2, "negative sphere count");
    if (s_has_bad_scene(scene)) return fail(-1, "null scene array");
    const RaysLayout R(sizeof(T), n, rec != nullptr);
    if (int rc = check_alias({{"idx", idx, R.idx_b}, {"rec", rec, R.rec_b}}, {{"rays", rays, R.rays_b}}, "the rays")) return rc;
    if (n == 0) return 0;               // nothing enqueued; this thread's last render is left alone
    DeviceGuard guard;
    release_last();
    RenderRec *rrec = nullptr;
    CtxPtr rctx;
    rtw_rays_params q = *p;
    int rc = stage_one_device<T>(p->device, scene, R.total, "the rays", {{R.off_rays, rays, R.rays_b}},
        [&](HostCtx *hc, char *base) {
            q.device = hc->device;
            return launch_rays<T>(hc->scene, base + R.off_rays, n, &q, base, rec ? base + R.off_rec : nullptr, hc->stream, &rrec, &rctx);
        },
        {0, idx, R.idx_b}, {{R.off_rec, rec, R.rec_b}}, "the records");
    if (!rc) rc = resolve_rec(rrec, &g_last.agg);
    if (!rc) g_last.per_device.emplace_back(q.device, g_last.agg.kernel_ms);
    if (rrec) release_rec(rctx, rrec, rc == 0);
    g_last.resolved = rc == 0;
    return rc;
}

// Radiance queries on host buffers (rtw_trace_rays_*): cast_rays_host's path with the radiance kernel -- a device buffer that holds the
// results and the rays (TraceRaysLayout); ONE H2D of the rays, ONE launch, ONE D2H of the results, then the counters of the record into
// this thread's last render.
template <typename T, typename SceneT>
int trace_rays_host(const SceneT *scene, const T *rays, int64_t n, const rtw_trace_params *p, double *out) {
    if (!p) return fail(-1, "null params");
    if (!scene || !rays || !out) return fail(-1, "null argument");
    if (int rc = validate_trace_rays(p, n)) return rc;
    if (scene->n < 0) return fail(-2, "negative sphere count");
    if (s_has_bad_scene(scene)) return fail(-1, "null scene array");
    const TraceRaysLayout R(sizeof(T), n);
    if (int rc = check_alias({{"out", out, R.out_b}}, {{"rays", rays, R.rays_b}}, "the rays")) return rc;
    if (n == 0) return 0;               // nothing enqueued; this thread's last render is left alone
    DeviceGuard guard;
    release_last();
    RenderRec *rrec = nullptr;
    CtxPtr rctx;
    rtw_trace_params q = *p;
    int rc = stage_one_device<T>(p->device, scene, R.total, "the rays", {{R.off_rays, rays, R.rays_b}},
        [&](HostCtx *hc, char *base) {
            q.device = hc->device;
            return launch_trace_rays<T>(hc->scene, base + R.off_rays, n, &q, base, hc->stream, &rrec, &rctx);
        },
        {0, out, R.out_b});
    if (!rc) rc = resolve_rec(rrec, &g_last.agg);
    if (!rc) g_last.per_device.emplace_back(q.device, g_last.agg.kernel_ms);
    if (rrec) release_rec(rctx, rrec, rc == 0);
    g_last.resolved = rc == 0;
    return rc;
}

// The launch sequence of render + feature pass + filter on a leased context (render_host_filtered, render_host_presented): the linear image, the
// features over all `nch` effective chunks and the filter with the caller's gamma into the regions R of hc->d_img.  `q`: the caller's params bound
// to the lease's device; rec / frec: the render's and the feature pass's records.
template <typename T, typename CamT>
int launch_filtered(HostCtx *hc, rtw_params &q, const CamT *cams, int32_t n_views, const uint64_t *seeds, int32_t gamma, const rtw_denoise_t *d, int nch, const DenoiseRegions<T> &R,
                    RenderRec **rec, CtxPtr *rctx, SideRec &frec) {
    char *base = (char *)hc->d_img;
    q.gamma = 0;
    rtw_denoise_t dd = *d;
    dd.gamma = gamma != 0; dd.device = hc->device;
    int rc = launch_render<T>(hc->scene, cams, n_views, seeds, &q, base, hc->stream, rec, rctx);
    if (!rc) rc = launch_features<T>(hc->scene, cams, n_views, seeds, &q, 0, nch, base + R.off_feat, hc->stream, &frec.rec, &frec.ctx);
    if (!rc) rc = R.launch(&dd, q.width, q.height, n_views, base, hc->stream);
    return rc;
}

// Render, feature pass over all N effective chunks and filter in one call (rtw_render_denoised_* / rtw_render_filtered_batch_*): the one-device
// path above with a device buffer that holds the linear image (the render with gamma 0), the features, the result (the filter with p->gamma) and
// the filter's workspace; 2 + 1 + levels launches for any number of views on the context's stream, ONE D2H.  rtw_stats() reports the render's record.
template <typename T, typename SceneT, typename CamT>
int render_host_filtered(const SceneT *scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_denoise_t *d, T *out) {
    if (!p) return fail(-1, "null params");
    if (!scene || !cams || !d || !out) return fail(-1, "null argument");
    int nch, cs;
    if (int rc = n_views ? validate_features_batch(cams, n_views, p, 0, 1, out, &nch, &cs) : validate_features(p, 0, 1, &nch, &cs)) return rc;
    if (int rc = n_views ? validate_filter_batch(d, p->width, p->height, n_views) : validate_denoise(d, p->width, p->height)) return rc;
    DeviceGuard guard;
    release_last();
    const DenoiseRegions<T> R(p->width, p->height, n_views);
    SideRec frec;                                             // (the feature pass's record)
    return render_one_device(p->device, scene, p, R.total, R.off_out, R.img_b, out, [&](HostCtx *hc, rtw_params &q, RenderRec **rec, CtxPtr *rctx) {
        return launch_filtered(hc, q, cams, n_views, seeds, p->gamma, d, nch, R, rec, rctx, frec);
    });
}

// Render and present in one call (rtw_render_presented_* / rtw_render_presented_batch_*): the one-device path above.  d null: the render with
// p->gamma as given into the head of the device buffer; d non-null: the launch sequence of render_host_filtered into its regions.  Then ONE
// launch of the present kernel over the device image of all views into a byte region behind everything else, and ONE D2H of those bytes.
template <typename T, typename SceneT, typename CamT>
int render_host_presented(const SceneT *scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_denoise_t *d, const rtw_present_t *pr,
                          uint8_t *out) {
    if (!p) return fail(-1, "null params");
    if (!scene || !cams || !pr || !out) return fail(-1, "null argument");
    int nch, cs;
    if (int rc = n_views ? validate_features_batch(cams, n_views, p, 0, 1, out, &nch, &cs) : validate_features(p, 0, 1, &nch, &cs)) return rc;
    if (d) { if (int rc = n_views ? validate_filter_batch(d, p->width, p->height, n_views) : validate_denoise(d, p->width, p->height)) return rc; }
    if (int rc = validate_present(pr, p->width, p->height, n_views)) return rc;
    DeviceGuard guard;
    release_last();
    const DenoiseRegions<T> R(p->width, p->height, n_views);
    const size_t pres_b = (size_t)rtw_present_bytes(p->width, p->height, pr->channels, n_views);
    DevLayout L{d ? R.total : R.img_b};                       // (the bytes: behind the filter's regions, or behind the image alone)
    const size_t off_img = d ? R.off_out : 0, off_pres = L.add(pres_b);
    SideRec frec;                                             // (the feature pass's record)
    // (render_one_device takes its precision from the type of `out` and hands the pointer to the D2H untyped: the bytes go out as they are)
    return render_one_device(p->device, scene, p, L.total, off_pres, pres_b, reinterpret_cast<T *>(out), [&](HostCtx *hc, rtw_params &q, RenderRec **rec, CtxPtr *rctx) {
        char *base = (char *)hc->d_img;
        rtw_present_t pp = *pr;
        pp.device = hc->device;
        int rc = d ? launch_filtered(hc, q, cams, n_views, seeds, p->gamma, d, nch, R, rec, rctx, frec)
                   : launch_render<T>(hc->scene, cams, n_views, seeds, &q, base, hc->stream, rec, rctx);
        if (!rc) rc = launch_present<T>(&pp, p->width, p->height, n_views, base + off_img, base + off_pres, hc->stream);
        return rc;
    });
}

// A small render, its feature pass, the full-size feature pass and the upsampler in one call (rtw_render_upsampled_* / rtw_render_upsampled_batch_*):
// the one-device path above with a device buffer that holds the small linear image (the render of q = p at the small size with gamma 0), the
// features of q over all of its chunks, the features of p over [0, hi_chunks), the result (the upsampler with p->gamma) and the workspace;
// 5 + levels launches for any number of views on the context's stream, ONE D2H.  rtw_stats() reports the small render's record.
template <typename T, typename SceneT, typename CamT>
int render_host_upsampled(const SceneT *scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, int32_t lo_width, int32_t lo_height,
                          const rtw_upsample_t *u, T *out) {
    if (!p) return fail(-1, "null params");
    if (!scene || !cams || !u || !out) return fail(-1, "null argument");
    rtw_params q = *p;
    q.width = lo_width; q.height = lo_height; q.gamma = 0;
    int nch_p, nch_q, cs;
    if (int rc = n_views ? validate_features_batch(cams, n_views, p, 0, 1, out, &nch_p, &cs) : validate_features(p, 0, 1, &nch_p, &cs)) return rc;
    if (int rc = n_views ? validate_features_batch(cams, n_views, &q, 0, 1, out, &nch_q, &cs) : validate_features(&q, 0, 1, &nch_q, &cs)) return rc;
    if (int rc = validate_upsample(u, lo_width, lo_height, p->width, p->height, n_views, (int)sizeof(T))) return rc;
    const int hi_chunks = u->hi_chunks ? u->hi_chunks : nch_p;
    if (int rc = check_chunk_range(0, hi_chunks, nch_p)) return rc;
    DeviceGuard guard;
    release_last();
    const UpsampleRegions<T> R(lo_width, lo_height, p->width, p->height, n_views);
    SideRec frec[2];                                          // (the two feature passes' records)
    return render_one_device(p->device, scene, p, R.total, R.off_out, R.out_b, out, [&](HostCtx *hc, rtw_params &pd, RenderRec **rec, CtxPtr *rctx) {
        char *base = (char *)hc->d_img;
        rtw_params qd = pd;
        qd.width = lo_width; qd.height = lo_height; qd.gamma = 0;
        rtw_upsample_t uu = *u;
        uu.gamma = p->gamma != 0; uu.device = hc->device;
        int rc = launch_render<T>(hc->scene, cams, n_views, seeds, &qd, base, hc->stream, rec, rctx);
        if (!rc) rc = launch_features<T>(hc->scene, cams, n_views, seeds, &qd, 0, nch_q, base + R.off_flo, hc->stream, &frec[0].rec, &frec[0].ctx);
        if (!rc) rc = launch_features<T>(hc->scene, cams, n_views, seeds, &pd, 0, hi_chunks, base + R.off_fhi, hc->stream, &frec[1].rec, &frec[1].ctx);
        if (!rc) rc = R.launch(&uu, lo_width, lo_height, p->width, p->height, n_views, base, hc->stream);
        return rc;
    });
}

// Render through the pinhole and apply the lens afterwards in one call: the one-device path above.  n_views == 0 (rtw_render_defocused_*: top 8,
// rtw_render_wide_aperture_*: top 32): one view; n_views >= 1 (rtw_render_lens_batch_*): that many views through the batched launch sequences
// that exist.  ONE render (gamma 0) and ONE feature pass over all chunks run through COPIES of the cameras with lens_radius = 0; with `d` ONE
// filter pass with gamma 0 (launch_filtered).  A batch alone then has ONE H2D of the lens table (built here: view v's lens is lens_radii[v] /
// focus_dists[v], null arrays: b's); a single call passes its constants as kernel arguments and has no table.  Then the stage -- six
// launches, two when max_radius <= 8 -- with p->gamma into a region behind the denoiser's, ONE D2H.  A lens radius of -1 is the camera's own
// (validate_lens_batch).  rtw_stats() reports the render's record.
template <typename T, typename SceneT, typename CamT>
int render_host_lens(int top, const SceneT *scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_denoise_t *d, const rtw_wide_aperture_t *b,
                     const double *lens_radii, const double *focus_dists, T *out) {
    if (!p) return fail(-1, "null params");
    if (!scene || !cams || !b || !out) return fail(-1, "null argument");
    int nch, cs;
    if (int rc = n_views ? validate_features_batch(cams, n_views, p, 0, 1, out, &nch, &cs) : validate_features(p, 0, 1, &nch, &cs)) return rc;
    if (scene->n < 0) return fail(-2, "negative sphere count");
    if (d) if (int rc = n_views ? validate_filter_batch(d, p->width, p->height, n_views) : validate_denoise(d, p->width, p->height)) return rc;
    const int32_t views = n_views ? n_views : 1;
    std::vector<rtw_defocus_t> lens;
    if (int rc = validate_lens_batch(b, cams, views, p->width, p->height, lens_radii, focus_dists, true, top, &lens)) return rc;
    rtw_wide_aperture_t bb = *b;
    bb.lens_radius = lens[0].lens_radius;                                      // (a single call's lens with the -1 resolved; a batch's lives in the table and this one is not read)
    bb.gamma = p->gamma != 0;                                                  // (b's gamma and device are judged, then replaced by p's)
    std::vector<CamT> pins(cams, cams + views);
    for (CamT &c : pins) c.lens_radius = 0;
    std::vector<T> table;
    if (n_views) { table.resize((size_t)n_views * 32); lens_table<T>(lens, pins.data(), p->width, table.data()); }
    DeviceGuard guard;
    release_last();
    const DenoiseRegions<T> R(p->width, p->height, n_views);
    const LensBatchLayout B(sizeof(T), p->width, p->height, bb.max_radius, n_views, n_views);
    DevLayout L{R.total};
    const size_t off_lens = L.add(B.out_b), off_work = L.add(B.work_b), off_tab = L.add(B.tab_b);
    SideRec frec;                                             // (the feature pass's record)
    return render_one_device(p->device, scene, p, L.total, off_lens, B.out_b, out, [&](HostCtx *hc, rtw_params &q, RenderRec **rec, CtxPtr *rctx) {
        char *base = (char *)hc->d_img;
        int rc;
        if (d) {
            rc = launch_filtered(hc, q, pins.data(), n_views, seeds, 0, d, nch, R, rec, rctx, frec);
        } else {
            q.gamma = 0;
            rc = launch_render<T>(hc->scene, pins.data(), n_views, seeds, &q, base, hc->stream, rec, rctx);
            if (!rc) rc = launch_features<T>(hc->scene, pins.data(), n_views, seeds, &q, 0, nch, base + R.off_feat, hc->stream, &frec.rec, &frec.ctx);
        }
        if (rc) return rc;
        if (n_views) HIP_TRY(hipMemcpyAsync(base + off_tab, table.data(), B.tab_b, hipMemcpyHostToDevice, hc->stream));
        bb.device = hc->device;
        const LensViews vb = lens_views(B, n_views, base + off_tab);
        return launch_wide_aperture<T>(&bb, pins.data(), p->width, p->height, base + (d ? R.off_out : 0), base + R.off_feat, base + off_work, base + off_lens, hc->stream, n_views ? &vb : nullptr);
    });
}

// N cameras along a path with history reuse (rtw_render_sequence_*): the one-device path above with a device buffer that holds the linear images
// (ONE batched render with gamma 0), the features (ONE batched pass over all chunks), the accumulated images (n_views temporal steps in view
// order, two states ping-pong) and, with `d`, the filtered images and the filter's workspace (ONE batched filter pass); 2 + n_views (+ 1 + levels)
// launches on the context's stream, ONE D2H.  p->gamma is applied by the last stage that runs.  rtw_stats() reports the render's record.
// `n` non-null (rtw_render_path_guided_*; d is then there): the steps carry moments (two moment planes ping-pong with the states), one noise
// launch follows each step (into view v of the noise region, before the ping-pong reuses that state: stream order) and the filter pass is the
// NOISE-GUIDED one over the N maps: 2 + 2*n_views + 1 + levels launches.  `guided` says only that the ENTRY POINT requires n and d, so that
// a null one is refused with -1 and not taken for the plain form; what runs is decided by n alone.
// `c` non-null (rtw_render_path_clamped_*): the steps behind view 0 are clamped steps, launch for launch.
// n_paths >= 1 (rtw_render_paths_*): n_views = n_steps * n_paths frames, step-major -- path s at step k is view k*n_paths + s of cams, seeds and
// out.  Still ONE render, ONE feature pass and ONE filter pass over all n_views frames; the table of all n_views camera constants
// (temporal_table: step k's previous cameras are step k-1's) goes up by ONE H2D from the context's pinned staging buffer, then n_steps
// BATCHED step launches (step k reads the table's entries [k*n_paths, (k+1)*n_paths); two sets of n_paths states -- with n, of moment planes
// -- ping-pong) and, with n, one batched noise launch behind each.  n_paths == 0 is the one path above, call for call.
template <typename T, typename SceneT, typename CamT>
int render_host_sequence(const SceneT *scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_temporal_t *t, const rtw_temporal_noise_t *n,
                         const rtw_denoise_t *d, T *out, const rtw_temporal_clamp_t *c = nullptr, bool guided = false, int32_t n_paths = 0) {
    if (!p) return fail(-1, "null params");
    if (!scene || !cams || !t || !out || (guided && (!n || !d))) return fail(-1, "null argument");
    int nch, cs;
    if (int rc = validate_features_batch(cams, n_views, p, 0, 1, out, &nch, &cs)) return rc;
    if (d) if (int rc = validate_filter_batch(d, p->width, p->height, n_views)) return rc;
    if (int rc = validate_temporal(t, p->width, p->height, (int)sizeof(T))) return rc;
    if (n) if (int rc = validate_temporal_noise(n, p->width, p->height, (int)sizeof(T))) return rc;
    if (c) if (int rc = validate_temporal_clamp(c)) return rc;
    if (n && ((t->flags & RTW_TEMPORAL_DEMODULATE) != 0) != ((d->flags & RTW_DENOISE_DEMODULATE) != 0))
        return fail(-2, "the DEMODULATE flags of t and d must agree (the noise map is relative to the state's luminance)");
    if (n_paths && (double)p->width * (double)p->height * (double)n_views >= (double)(1ll << 39))         // (without d nothing above has applied the batch's size rule)
        return fail(-5, "batch too large for one call: %d frames of %d x %d pixels", n_views, p->width, p->height);
    DeviceGuard guard;
    release_last();
    const size_t np = n_paths ? (size_t)n_paths : 1;          // paths per step launch
    const int32_t n_steps = n_paths ? n_views / n_paths : n_views;
    const MomentRegions<T> R(p->width, p->height, (size_t)n_views, d != nullptr, np, n != nullptr);
    const size_t dev_b = n_paths ? R.total_p : n ? R.total_m : R.total;
    SideRec frec;                                             // (the feature pass's record)
    return render_one_device(p->device, scene, p, dev_b, d ? R.off_flt : R.off_acc, R.img_b, out, [&](HostCtx *hc, rtw_params &q, RenderRec **rec, CtxPtr *rctx) {
        char *base = (char *)hc->d_img;
        q.gamma = 0;
        rtw_temporal_t tt = *t;
        tt.gamma = d ? 0 : (p->gamma != 0); tt.device = hc->device;
        int rc = launch_render<T>(hc->scene, cams, n_views, seeds, &q, base, hc->stream, rec, rctx);
        if (!rc) rc = launch_features<T>(hc->scene, cams, n_views, seeds, &q, 0, nch, base + R.off_feat, hc->stream, &frec.rec, &frec.ctx);
        if (!rc && n_paths) {
            // the whole table: step 0's entries are first frames', step k's previous cameras are step k-1's
            if ((rc = ensure_stage(hc, R.tab_b))) return rc;
            T *tab = (T *)hc->h_stage;
            temporal_table<T, CamT>(cams, nullptr, n_paths, tab);
            if (n_steps > 1) temporal_table<T>(cams + n_paths, cams, (int64_t)(n_steps - 1) * n_paths, tab + 32 * np);
            HIP_TRY(hipMemcpyAsync(base + R.off_tab, tab, R.tab_b, hipMemcpyHostToDevice, hc->stream));
        }
        const size_t feat_frame_b = R.feat_b / (size_t)n_views;
        for (int v = 0; v < n_steps && !rc; ++v) {
            const size_t f = (size_t)v * np;                  // the step's first frame
            rc = launch_temporal<T>(&tt, n_paths ? nullptr : cams + v, n_paths || !v ? nullptr : cams + (v - 1), n_paths, n_paths ? base + R.off_tab + f * 32 * sizeof(T) : nullptr, p->width,
                                    p->height, base + f * R.frame_b, base + R.off_feat + f * feat_frame_b, v ? base + R.off_st[(v & 1) ^ 1] : nullptr, base + R.off_st[v & 1],
                                    base + R.off_acc + f * R.frame_b, hc->stream, n && v ? base + R.off_mo[(v & 1) ^ 1] : nullptr, n ? base + R.off_mo[v & 1] : nullptr, c);
            if (!rc && n) rc = launch_temporal_noise<T>(n, p->width, p->height, n_paths, base + R.off_st[v & 1], base + R.off_mo[v & 1], base + R.off_noise + f * R.noise_b, hc->stream);
        }
        if (!rc && d) {
            rtw_denoise_t dd = *d;
            dd.gamma = p->gamma != 0; dd.device = hc->device;
            rc = launch_denoise<T>(&dd, p->width, p->height, n_views, base + R.off_acc, base + R.off_feat, base + R.off_flt, base + R.off_work, hc->stream,
                                   n ? base + R.off_noise : nullptr);
        }
        return rc;
    });
}

// rtw_render_paths_*: n_paths paths x n_steps steps, step-major, in any of the sequence's forms -- c null: plain steps; n (d is then required): the
// guided form.  The counts and their product first; everything else is the sequence's own check of n_steps*n_paths views.
template <typename T, typename SceneT, typename CamT>
int render_host_paths(const SceneT *scene, const CamT *cams, int32_t n_paths, int32_t n_steps, const uint64_t *seeds, const rtw_params *p, const rtw_temporal_t *t,
                      const rtw_temporal_clamp_t *c, const rtw_temporal_noise_t *n, const rtw_denoise_t *d, T *out) {
    if (!p) return fail(-1, "null params");
    if (!scene || !cams || !t || !out) return fail(-1, "null argument");
    if (n_paths < 1 || n_steps < 1) return fail(-2, "n_paths and n_steps must be >= 1 (got %d, %d)", n_paths, n_steps);
    if ((int64_t)n_paths * n_steps > INT32_MAX) return fail(-2, "n_steps * n_paths must fit in 32 bits (got %d * %d)", n_steps, n_paths);
    if (n && !d) return fail(-2, "a noise map (n) guides the filter: d is required with it");
    return render_host_sequence<T>(scene, cams, n_paths * n_steps, seeds, p, t, n, d, out, c, n != nullptr, n_paths);
}

// rtw_render_path_clamped_*: the sequence (n null; d optional) or the guided sequence (n and d) with clamped steps.
template <typename T, typename SceneT, typename CamT>
int render_host_sequence_clamped(const SceneT *scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_temporal_t *t, const rtw_temporal_clamp_t *c,
                                 const rtw_temporal_noise_t *n, const rtw_denoise_t *d, T *out) {
    if (!p) return fail(-1, "null params");
    if (!c) return fail(-1, "null temporal clamp parameters");
    if (n && !d) return fail(-2, "a noise map (n) guides the filter: d is required with it");
    return render_host_sequence<T>(scene, cams, n_views, seeds, p, t, n, d, out, c, n != nullptr);
}


// n_frames scenes and cameras with history reuse across the spheres' motion (rtw_render_animation_*): the sequence above for a scene that
// changes from frame to frame, so what it batches over one scene runs per frame here, all on the leased context's stream: the frame's
// scene uploaded (reused while its bytes are those of the frame before; an upload it replaces is kept until the stream has drained, since
// the launches behind it may still read it), the render with gamma 0 and seeds[v] (null: p->seed), the feature pass over all chunks, from
// frame 1 on the motion table against the frame before (host arithmetic into the context's pinned staging buffer, every frame's table at
// its own offset, one H2D each) and the motion pass, then the step (two states ping-pong; `c`: clamped steps) -- 3 launches for frame 0, 4 for
// every other.  The device buffer holds the sequence's regions, ONE motion plane and ONE table behind them (stream order lets every frame
// reuse both).  With `d` ONE batched filter pass over all frames, then ONE D2H.  p->gamma is applied by the last stage that runs.
// rtw_stats(): the counters of all frames' renders summed, the times of the slowest.
// `b` non-null (rtw_render_blurred_*; `blurred` says only that the ENTRY POINT requires it): every stage above runs with gamma 0,
// every frame keeps a motion plane of its own, and behind the last of them the motion-blur stage runs per frame with p->gamma -- three
// launches for every frame from 1 on, the one pass-through launch for frame 0 -- into a region of n_frames frames behind the table, with ONE
// workspace (stream order lets every frame reuse it); the D2H reads that region.  Without `b` the buffer and the launches are what they were.
// (The stage path with frame 0's scene; not render_one_device: that uploads one scene and resolves one record.)
template <typename T, typename SceneT, typename CamT>
int render_host_animation(const SceneT *scenes, const CamT *cams, int32_t n_frames, const uint64_t *seeds, const rtw_params *p, const rtw_temporal_t *t, const rtw_temporal_clamp_t *c,
                          const rtw_denoise_t *d, T *out, const rtw_velocity_blur_t *b = nullptr, bool blurred = false) {
    if (!p) return fail(-1, "null params");
    if (!scenes || !cams || !t || !out || (blurred && !b)) return fail(-1, "null argument");
    if (n_frames < 1) return fail(-2, "n_frames must be >= 1 (got %d)", n_frames);
    int nch, cs;
    if (int rc = validate_features_batch(cams, n_frames, p, 0, 1, out, &nch, &cs)) return rc;
    if (d) if (int rc = validate_filter_batch(d, p->width, p->height, n_frames)) return rc;
    if (int rc = validate_temporal(t, p->width, p->height, (int)sizeof(T))) return rc;
    if (c) if (int rc = validate_temporal_clamp(c)) return rc;
    if (b) if (int rc = validate_motion_blur(b, p->width, p->height, (int)sizeof(T))) return rc;
    rtw_params pm = *p;                                       // the motion pass reads the frame, the device and the numerics bits
    pm.flags &= RTW_FLAG_GROUP_CULL | RTW_FLAG_SCAN_VALU | RTW_FLAG_NUMERICS_CONTRACT | RTW_FLAG_NUMERICS_REFERENCE_FMA2;
    if (int rc = validate_motion(&pm, (int)sizeof(T))) return rc;
    size_t tab_max = 0, tab_sum = 0;                          // (a table's bytes are a multiple of 16: the frames' tables lie one behind the other in the staging buffer)
    for (int v = 0; v < n_frames; ++v) {
        if (scenes[v].n < 0) return fail(-2, "negative sphere count (frame %d)", v);
        if (s_has_bad_scene(&scenes[v])) return fail(-1, "null scene array (frame %d)", v);
        const size_t tab_b = (size_t)scenes[v].n * 4 * sizeof(T);
        if (v) { tab_max = std::max(tab_max, tab_b); tab_sum += tab_b; }
    }
    DeviceGuard guard;
    release_last();
    const TemporalRegions<T> R(p->width, p->height, (size_t)n_frames, d != nullptr);
    const size_t mo_b = (size_t)p->width * (size_t)p->height * 4 * sizeof(T), feat_frame_b = R.feat_b / (size_t)n_frames;
    DevLayout B{R.total};                                     // (behind the sequence's regions: the motion planes, the table, with b the blurred frames and the blur's workspace)
    const size_t off_mo = B.add(mo_b * (b ? (size_t)n_frames : 1)), off_tab = B.add(tab_max);
    const size_t off_blur = b ? B.add(R.img_b) : 0, off_bwork = b ? B.add((size_t)rtw_velocity_blur_work_bytes(p->width, p->height, (int32_t)sizeof(T))) : 0;
    std::vector<ScenePtr> replaced;                           // (outlives the lease: the stream has drained when these are freed)
    std::vector<RenderRec *> recs((size_t)n_frames, nullptr);
    std::vector<CtxPtr> rctx((size_t)n_frames);
    std::vector<SideRec> frecs((size_t)n_frames);
    rtw_params q = *p;
    q.n_devices = 0; q.device_ids = nullptr; q.gamma = 0;
    int rc = stage_one_device<T>(p->device, &scenes[0], B.total, "", {}, [&](HostCtx *hc, char *base) {
        if (int rc = ensure_stage(hc, tab_sum)) return rc;
        q.device = pm.device = hc->device;
        rtw_temporal_t tt = *t;
        tt.gamma = (d || b) ? 0 : (p->gamma != 0); tt.device = hc->device;
        std::vector<unsigned char> key;
        int rc = 0;
        size_t stage_off = 0;
        for (int v = 0; v < n_frames && !rc; ++v) {
            const SceneT *scene = scenes + v;                     // (frame 0's is the lease's)
            if (v) scene_key_of(scene, sizeof(T) == 8, key);
            if (v && (rc = ensure_scene<T>(hc, scene, key, &replaced))) break;
            if (seeds) q.seed = seeds[v];
            char *img = base + (size_t)v * R.frame_b, *feat = base + R.off_feat + (size_t)v * feat_frame_b, *plane = base + off_mo + (b ? (size_t)v * mo_b : 0);
            rc = launch_render<T>(hc->scene, cams + v, 0, nullptr, &q, img, hc->stream, &recs[v], &rctx[v]);
            if (!rc) rc = launch_features<T>(hc->scene, cams + v, 0, nullptr, &q, 0, nch, feat, hc->stream, &frecs[v].rec, &frecs[v].ctx);
            if (!rc && v) {
                const size_t tab_b = (size_t)scene->n * 4 * sizeof(T);
                T *tab = (T *)((char *)hc->h_stage + stage_off);
                stage_off += tab_b;
                if (tab_b) {
                    rc = motion_table<T>(scene - 1, scene, tab);
                    if (!rc) if (hipError_t e = hipMemcpyAsync(base + off_tab, tab, tab_b, hipMemcpyHostToDevice, hc->stream); e != hipSuccess)
                        rc = fail((int)e, "upload of the motion table failed: %s", hipGetErrorString(e));
                }
                if (!rc) rc = launch_motion<T>(hc->scene, cams + v, &pm, tab_b ? base + off_tab : nullptr, plane, hc->stream);
            }
            if (!rc) rc = launch_temporal<T>(&tt, cams + v, v ? cams + (v - 1) : nullptr, 0, nullptr, p->width, p->height, img, feat, v ? base + R.off_st[(v & 1) ^ 1] : nullptr,
                                             base + R.off_st[v & 1], base + R.off_acc + (size_t)v * R.frame_b, hc->stream, nullptr, nullptr, c, v ? plane : nullptr);
        }
        if (!rc && d) {
            rtw_denoise_t dd = *d;
            dd.gamma = b ? 0 : (p->gamma != 0); dd.device = hc->device;
            rc = launch_denoise<T>(&dd, p->width, p->height, n_frames, base + R.off_acc, base + R.off_feat, base + R.off_flt, base + R.off_work, hc->stream);
        }
        if (b) {
            rtw_velocity_blur_t bb = *b;
            bb.gamma = p->gamma != 0; bb.device = hc->device;
            for (int v = 0; v < n_frames && !rc; ++v)
                rc = launch_motion_blur<T>(&bb, cams + v, v ? cams + (v - 1) : nullptr, p->width, p->height, base + (d ? R.off_flt : R.off_acc) + (size_t)v * R.frame_b,
                                           base + R.off_feat + (size_t)v * feat_frame_b, base + off_mo + (size_t)v * mo_b, base + off_bwork, base + off_blur + (size_t)v * R.frame_b, hc->stream);
        }
        return rc;
    }, {b ? off_blur : d ? R.off_flt : R.off_acc, out, R.img_b});
    for (int v = 0; v < n_frames; ++v)
        if (recs[v]) { if (!rc) rc = resolve_rec(recs[v], &g_last.agg); release_rec(rctx[v], recs[v], rc == 0); }
    if (!rc) g_last.per_device.emplace_back(q.device, g_last.agg.kernel_ms);
    g_last.resolved = rc == 0;
    return rc;
}

// What an accumulator holds, denoised (rtw_accum_filtered_f32/_f64): the gamma-0 resolve (per tile for an adaptive accumulator), the feature
// pass over exactly the samples it holds, with `guided` its noise map and the noise-guided filter (else the plain one), all on the
// accumulator's device in a leased context's buffer and stream, ONE D2H.  The accumulator is only read; every step orders itself behind
// its event.  rtw_stats() reports the feature pass's record.  (The stage path with the record resolved behind it: the lease has no scene to upload.)
// n_views != 0 (rtw_accum_filtered_batch_*): the same for the n_views accumulators behind `accums` with cams[v] / seeds[v] -- ONE batched
// resolve, ONE batched feature launch, ONE batched noise launch and the batched filter, 4 + levels launches and ONE D2H for any number of views.
template <typename T, typename CamT>
int accum_filtered_host(rtw_scene_handle scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_denoise_t *d, const rtw_accum_handle *accums,
                        int32_t guided, T *out) {
    constexpr bool f64 = sizeof(T) == 8;
    if (!p) return fail(-1, "null params");
    if (!scene || !cams || !d || !accums || !out) return fail(-1, "null argument");
    if (n_views) { if (int rc = validate_accum_array(accums, n_views)) return rc; }
    else if (!accums[0]) return fail(-1, "null argument");
    if (guided != 0 && guided != 1) return fail(-2, "guided must be 0 or 1 (got %d)", guided);
    int nch, cs;                                                   // (the render's and the filter's own checks before a handle is looked at)
    if (int rc = n_views ? validate_features_batch(cams, n_views, p, 0, 1, out, &nch, &cs) : validate_features(p, 0, 1, &nch, &cs)) return rc;
    if (int rc = n_views ? validate_filter_batch(d, p->width, p->height, n_views) : validate_denoise(d, p->width, p->height)) return rc;
    if (int rc = n_views ? validate_accum_features_batch(scene, cams, n_views, seeds, p, accums) : validate_accum_features(scene, cams, p, accums[0])) return rc;
    if (n_views) if (int rc = validate_accum_resolve_batch(accums, n_views, f64)) return rc;
    if (guided) if (int rc = n_views ? validate_accum_noise_batch(accums, n_views, f64) : validate_accum_noise(accums[0], f64)) return rc;
    DeviceGuard guard;
    release_last();
    const DenoiseRegions<T> R(p->width, p->height, n_views);
    DevLayout B{R.total};                                     // (the noise maps: behind the filter's regions)
    const size_t off_noise = B.add((size_t)std::max(n_views, 1) * (size_t)p->width * (size_t)p->height * sizeof(T));
    RenderRec *frec = nullptr;
    CtxPtr fctx;
    int rc = stage_one_device<T>(accum_device_of(accums[0]), nullptr, B.total, "", {}, [&](HostCtx *hc, char *base) {
        rtw_denoise_t dd = *d;
        dd.gamma = p->gamma != 0; dd.device = hc->device;
        int rc;
        if (n_views) {
            rc = enqueue_accum_resolve_batch(accums, n_views, f64, 0, base, hc->stream);
            if (!rc) rc = enqueue_accum_features_batch(scene, cams, n_views, seeds, p, accums, base + R.off_feat, hc->stream, &frec, &fctx);
            if (!rc && guided) rc = enqueue_accum_noise_batch(accums, n_views, f64, base + off_noise, hc->stream);
        } else {
            rc = enqueue_accum_resolve(accums[0], f64, 0, base, hc->stream);
            if (!rc) rc = enqueue_accum_features(scene, cams, p, accums[0], base + R.off_feat, hc->stream, &frec, &fctx);
            if (!rc && guided) rc = enqueue_accum_noise(accums[0], f64, base + off_noise, hc->stream);
        }
        if (!rc) rc = R.launch(&dd, p->width, p->height, n_views, base, hc->stream, guided ? base + off_noise : nullptr);
        return rc;
    }, {R.off_out, out, R.img_b});
    if (!rc) rc = resolve_rec(frec, &g_last.agg);
    if (!rc) g_last.per_device.emplace_back(frec->device, g_last.agg.kernel_ms);
    if (frec) release_rec(fctx, frec, rc == 0);
    g_last.resolved = rc == 0;
    return rc;
}

}  // namespace rtwh

using namespace rtwh;

// ---- the host-buffer entry points of the C ABI (include/rtw_hip.h) ------------------------------------------------------
extern "C" {

int rtw_render_f32(const rtw_scene_f32 *s, const rtw_camera_f32 *c, const rtw_params *p, float *out) { return render_host<float>(s, c, p, out); }
int rtw_render_f64(const rtw_scene_f64 *s, const rtw_camera_f64 *c, const rtw_params *p, double *out) { return render_host<double>(s, c, p, out); }
int rtw_render_batch_f32(const rtw_scene_f32 *s, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, float *out) {
    return render_host_batch<float>(s, cams, n_views, seeds, p, out);
}
int rtw_render_batch_f64(const rtw_scene_f64 *s, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, double *out) {
    return render_host_batch<double>(s, cams, n_views, seeds, p, out);
}

int rtw_render_features_f32(const rtw_scene_f32 *s, const rtw_camera_f32 *c, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, float *out) {
    return render_host_features<float>(s, c, 0, nullptr, p, chunk_begin, chunk_count, out);
}
int rtw_render_features_f64(const rtw_scene_f64 *s, const rtw_camera_f64 *c, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, double *out) {
    return render_host_features<double>(s, c, 0, nullptr, p, chunk_begin, chunk_count, out);
}
int rtw_render_features_batch_f32(const rtw_scene_f32 *s, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, int32_t chunk_begin,
                                  int32_t chunk_count, float *out) {
    return render_host_features<float>(s, cams, batch_views(n_views), seeds, p, chunk_begin, chunk_count, out);
}
int rtw_render_features_batch_f64(const rtw_scene_f64 *s, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, int32_t chunk_begin,
                                  int32_t chunk_count, double *out) {
    return render_host_features<double>(s, cams, batch_views(n_views), seeds, p, chunk_begin, chunk_count, out);
}


int rtw_render_denoised_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cam, const rtw_params *p, const rtw_denoise_t *d, float *out) {
    return render_host_filtered<float>(scene, cam, 0, nullptr, p, d, out);
}
int rtw_render_denoised_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cam, const rtw_params *p, const rtw_denoise_t *d, double *out) {
    return render_host_filtered<double>(scene, cam, 0, nullptr, p, d, out);
}
int rtw_render_filtered_batch_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_denoise_t *d,
                                  float *out) {
    return render_host_filtered<float>(scene, cams, batch_views(n_views), seeds, p, d, out);
}
int rtw_render_filtered_batch_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_denoise_t *d,
                                  double *out) {
    return render_host_filtered<double>(scene, cams, batch_views(n_views), seeds, p, d, out);
}

int rtw_render_presented_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cam, const rtw_params *params, const rtw_denoise_t *d, const rtw_present_t *p, uint8_t *out) {
    return render_host_presented<float>(scene, cam, 0, nullptr, params, d, p, out);
}
int rtw_render_presented_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cam, const rtw_params *params, const rtw_denoise_t *d, const rtw_present_t *p, uint8_t *out) {
    return render_host_presented<double>(scene, cam, 0, nullptr, params, d, p, out);
}
int rtw_render_presented_batch_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *params, const rtw_denoise_t *d,
                                   const rtw_present_t *p, uint8_t *out) {
    return render_host_presented<float>(scene, cams, batch_views(n_views), seeds, params, d, p, out);
}
int rtw_render_presented_batch_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *params, const rtw_denoise_t *d,
                                   const rtw_present_t *p, uint8_t *out) {
    return render_host_presented<double>(scene, cams, batch_views(n_views), seeds, params, d, p, out);
}

int rtw_render_upsampled_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cam, const rtw_params *p, int32_t lo_width, int32_t lo_height, const rtw_upsample_t *u, float *out) {
    return render_host_upsampled<float>(scene, cam, 0, nullptr, p, lo_width, lo_height, u, out);
}
int rtw_render_upsampled_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cam, const rtw_params *p, int32_t lo_width, int32_t lo_height, const rtw_upsample_t *u, double *out) {
    return render_host_upsampled<double>(scene, cam, 0, nullptr, p, lo_width, lo_height, u, out);
}
int rtw_render_upsampled_batch_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, int32_t lo_width,
                                   int32_t lo_height, const rtw_upsample_t *u, float *out) {
    return render_host_upsampled<float>(scene, cams, batch_views(n_views), seeds, p, lo_width, lo_height, u, out);
}
int rtw_render_upsampled_batch_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, int32_t lo_width,
                                   int32_t lo_height, const rtw_upsample_t *u, double *out) {
    return render_host_upsampled<double>(scene, cams, batch_views(n_views), seeds, p, lo_width, lo_height, u, out);
}

int rtw_first_hit_motion_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cam, const rtw_params *p, const float *table, float *motion) {
    return render_host_motion<float>(scene, cam, p, table, motion);
}
int rtw_first_hit_motion_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cam, const rtw_params *p, const double *table, double *motion) {
    return render_host_motion<double>(scene, cam, p, table, motion);
}
int rtw_cast_rays_f32(const rtw_scene_f32 *scene, const float *rays, int64_t n, const rtw_rays_params *p, int32_t *idx, float *rec) {
    return cast_rays_host<float>(scene, rays, n, p, idx, rec);
}
int rtw_cast_rays_f64(const rtw_scene_f64 *scene, const double *rays, int64_t n, const rtw_rays_params *p, int32_t *idx, double *rec) {
    return cast_rays_host<double>(scene, rays, n, p, idx, rec);
}
int rtw_trace_rays_f32(const rtw_scene_f32 *scene, const float *rays, int64_t n, const rtw_trace_params *p, double *out) {
    return trace_rays_host<float>(scene, rays, n, p, out);
}
int rtw_trace_rays_f64(const rtw_scene_f64 *scene, const double *rays, int64_t n, const rtw_trace_params *p, double *out) {
    return trace_rays_host<double>(scene, rays, n, p, out);
}
int rtw_render_animation_f32(const rtw_scene_f32 *scenes, const rtw_camera_f32 *cams, int32_t n_frames, const uint64_t *seeds, const rtw_params *p, const rtw_temporal_t *t,
                             const rtw_temporal_clamp_t *c, const rtw_denoise_t *d, float *out) {
    return render_host_animation<float>(scenes, cams, n_frames, seeds, p, t, c, d, out);
}
int rtw_render_animation_f64(const rtw_scene_f64 *scenes, const rtw_camera_f64 *cams, int32_t n_frames, const uint64_t *seeds, const rtw_params *p, const rtw_temporal_t *t,
                             const rtw_temporal_clamp_t *c, const rtw_denoise_t *d, double *out) {
    return render_host_animation<double>(scenes, cams, n_frames, seeds, p, t, c, d, out);
}
int rtw_render_blurred_f32(const rtw_scene_f32 *scenes, const rtw_camera_f32 *cams, int32_t n_frames, const uint64_t *seeds, const rtw_params *p, const rtw_temporal_t *t,
                                     const rtw_temporal_clamp_t *c, const rtw_denoise_t *d, const rtw_velocity_blur_t *b, float *out) {
    return render_host_animation<float>(scenes, cams, n_frames, seeds, p, t, c, d, out, b, true);
}
int rtw_render_blurred_f64(const rtw_scene_f64 *scenes, const rtw_camera_f64 *cams, int32_t n_frames, const uint64_t *seeds, const rtw_params *p, const rtw_temporal_t *t,
                                     const rtw_temporal_clamp_t *c, const rtw_denoise_t *d, const rtw_velocity_blur_t *b, double *out) {
    return render_host_animation<double>(scenes, cams, n_frames, seeds, p, t, c, d, out, b, true);
}
int rtw_render_defocused_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cam, const rtw_params *p, const rtw_denoise_t *d, const rtw_defocus_t *b, float *out) {
    return render_host_lens<float>(RTW_DEFOCUS_MAX_RADIUS, scene, cam, 0, nullptr, p, d, AsWideAperture(b).ptr, nullptr, nullptr, out);
}
int rtw_render_defocused_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cam, const rtw_params *p, const rtw_denoise_t *d, const rtw_defocus_t *b, double *out) {
    return render_host_lens<double>(RTW_DEFOCUS_MAX_RADIUS, scene, cam, 0, nullptr, p, d, AsWideAperture(b).ptr, nullptr, nullptr, out);
}
int rtw_render_wide_aperture_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cam, const rtw_params *p, const rtw_denoise_t *d, const rtw_wide_aperture_t *b, float *out) {
    return render_host_lens<float>(RTW_WIDE_APERTURE_MAX_RADIUS, scene, cam, 0, nullptr, p, d, b, nullptr, nullptr, out);
}
int rtw_render_wide_aperture_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cam, const rtw_params *p, const rtw_denoise_t *d, const rtw_wide_aperture_t *b, double *out) {
    return render_host_lens<double>(RTW_WIDE_APERTURE_MAX_RADIUS, scene, cam, 0, nullptr, p, d, b, nullptr, nullptr, out);
}
int rtw_render_lens_batch_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_denoise_t *d,
                                       const rtw_wide_aperture_t *b, const double *lens_radii, const double *focus_dists, float *out) {
    return render_host_lens<float>(RTW_WIDE_APERTURE_MAX_RADIUS, scene, cams, batch_views(n_views), seeds, p, d, b, lens_radii, focus_dists, out);
}
int rtw_render_lens_batch_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_denoise_t *d,
                                       const rtw_wide_aperture_t *b, const double *lens_radii, const double *focus_dists, double *out) {
    return render_host_lens<double>(RTW_WIDE_APERTURE_MAX_RADIUS, scene, cams, batch_views(n_views), seeds, p, d, b, lens_radii, focus_dists, out);
}
int rtw_render_path_clamped_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_temporal_t *t,
                                 const rtw_temporal_clamp_t *c, const rtw_temporal_noise_t *n, const rtw_denoise_t *d, float *out) {
    return render_host_sequence_clamped<float>(scene, cams, batch_views(n_views), seeds, p, t, c, n, d, out);
}
int rtw_render_path_clamped_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_temporal_t *t,
                                 const rtw_temporal_clamp_t *c, const rtw_temporal_noise_t *n, const rtw_denoise_t *d, double *out) {
    return render_host_sequence_clamped<double>(scene, cams, batch_views(n_views), seeds, p, t, c, n, d, out);
}
int rtw_render_paths_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_paths, int32_t n_steps, const uint64_t *seeds, const rtw_params *p, const rtw_temporal_t *t,
                         const rtw_temporal_clamp_t *c, const rtw_temporal_noise_t *n, const rtw_denoise_t *d, float *out) {
    return render_host_paths<float>(scene, cams, n_paths, n_steps, seeds, p, t, c, n, d, out);
}
int rtw_render_paths_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_paths, int32_t n_steps, const uint64_t *seeds, const rtw_params *p, const rtw_temporal_t *t,
                         const rtw_temporal_clamp_t *c, const rtw_temporal_noise_t *n, const rtw_denoise_t *d, double *out) {
    return render_host_paths<double>(scene, cams, n_paths, n_steps, seeds, p, t, c, n, d, out);
}
int rtw_render_path_guided_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_temporal_t *t,
                                   const rtw_temporal_noise_t *n, const rtw_denoise_t *d, float *out) {
    return render_host_sequence<float>(scene, cams, batch_views(n_views), seeds, p, t, n, d, out, nullptr, true);
}
int rtw_render_path_guided_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_temporal_t *t,
                                   const rtw_temporal_noise_t *n, const rtw_denoise_t *d, double *out) {
    return render_host_sequence<double>(scene, cams, batch_views(n_views), seeds, p, t, n, d, out, nullptr, true);
}
int rtw_render_sequence_f32(const rtw_scene_f32 *scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_temporal_t *t,
                            const rtw_denoise_t *d, float *out) {
    return render_host_sequence<float>(scene, cams, batch_views(n_views), seeds, p, t, nullptr, d, out);
}
int rtw_render_sequence_f64(const rtw_scene_f64 *scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_temporal_t *t,
                            const rtw_denoise_t *d, double *out) {
    return render_host_sequence<double>(scene, cams, batch_views(n_views), seeds, p, t, nullptr, d, out);
}

int rtw_accum_filtered_f32(rtw_scene_handle scene, const rtw_camera_f32 *cam, const rtw_params *p, const rtw_denoise_t *d, rtw_accum_handle accum, int32_t guided, float *out) {
    return accum_filtered_host<float>(scene, cam, 0, nullptr, p, d, &accum, guided, out);
}
int rtw_accum_filtered_f64(rtw_scene_handle scene, const rtw_camera_f64 *cam, const rtw_params *p, const rtw_denoise_t *d, rtw_accum_handle accum, int32_t guided, double *out) {
    return accum_filtered_host<double>(scene, cam, 0, nullptr, p, d, &accum, guided, out);
}
int rtw_accum_filtered_batch_f32(rtw_scene_handle scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_denoise_t *d,
                                 const rtw_accum_handle *accums, int32_t guided, float *out) {
    return accum_filtered_host<float>(scene, cams, batch_views(n_views), seeds, p, d, accums, guided, out);
}
int rtw_accum_filtered_batch_f64(rtw_scene_handle scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_denoise_t *d,
                                 const rtw_accum_handle *accums, int32_t guided, double *out) {
    return accum_filtered_host<double>(scene, cams, batch_views(n_views), seeds, p, d, accums, guided, out);
}

}  // extern "C"
