// rtw_accum.hip -- progressive render (include/rtw_hip.h rtw_accum_*, rtw_render_accum_*): the accumulator object (rtw_accum.hpp), the
// checks of a pass, merge and resolve, the export / import blob, the adaptive render (rtw_render_adaptive_*): the host loop of passes over
// the tiles still active, and the read-only passes that make an accumulator the denoiser's input.  Host code only: every kernel and its
// launch is in rtw_accum_kernels.hip.
//
// An accumulator is W x H pixels x 8 uint64 in HBM (the job slot's own layout, rtw_kernels.hpp AccumArgs) plus, on the host, the render it
// is bound to and the chunk ranges it already holds.  Every sample is a signed 64.64 integer and integer addition is associative, so ANY
// partition of a render's chunks into passes -- in any order, in any mix of scan modes and job sizes, on one accumulator or merged from
// several -- resolves to the bits of the single render.  Nothing here needs an atomic: within a launch one workgroup owns a pixel, and
// everything that touches an accumulator is ordered behind its event (`ev`: recorded after every pass / merge / reset, waited for by
// whatever comes next on whichever stream).
#include "rtw_accum.hpp"

namespace rtwh {

namespace {

#define RTW_ACCUM_BLOB_VERSION 1u
struct BlobHeader {
    char magic[8];                  // "RTWACCUM"
    uint32_t version, header_bytes; // RTW_ACCUM_BLOB_VERSION, sizeof(BlobHeader)
    int32_t width, height, bound, n_ranges;
    AccumBind bind;
};
static_assert(sizeof(BlobHeader) == 248, "the blob header is part of the file format");
// followed by n_ranges x (int32 begin, int32 end), then width * height * 8 uint64 (little endian, like the device)

size_t n_pixels(const rtw_accum *a) { return (size_t)a->width * (size_t)a->height; }

long long samples_in(const AccumBind &b, long long begin, long long end) {
    return std::min<long long>(b.spp, end * b.chunk_spp) - std::min<long long>(b.spp, begin * b.chunk_spp);
}
long long samples_done(const rtw_accum *a) {
    long long s = 0;
    if (a->bound) for (auto &r : a->ranges) s += samples_in(a->bind, r.first, r.second);
    return s;
}
int chunks_done(const rtw_accum *a) {
    int c = 0;
    for (auto &r : a->ranges) c += r.second - r.first;
    return c;
}
bool overlaps(const std::vector<std::pair<int32_t, int32_t>> &rs, int32_t b, int32_t e) {
    for (auto &r : rs) if (b < r.second && r.first < e) return true;
    return false;
}
void add_range(std::vector<std::pair<int32_t, int32_t>> &rs, int32_t b, int32_t e) {
    rs.emplace_back(b, e);
    std::sort(rs.begin(), rs.end());
    std::vector<std::pair<int32_t, int32_t>> out;
    for (auto &r : rs) {
        if (!out.empty() && out.back().second == r.first) out.back().second = r.second;
        else out.push_back(r);
    }
    rs.swap(out);
}
bool same_render(const AccumBind &x, const AccumBind &y) { return memcmp(&x, &y, sizeof(AccumBind)) == 0; }

template <typename CamT>
void make_bind(AccumBind *b, rtw_scene_handle scene, const CamT *cam, const rtw_params *p, int nch, int cs) {
    memset(b, 0, sizeof *b);
    b->is_f64 = sizeof(CamT) == sizeof(rtw_camera_f64);
    b->spp = p->spp; b->chunk_spp = cs; b->n_chunks = nch; b->max_depth = p->max_depth;
    b->numerics = p->flags & (RTW_FLAG_NUMERICS_CONTRACT | RTW_FLAG_NUMERICS_REFERENCE_FMA2);
    b->seed = p->seed; b->scene_hash = scene->content_hash;
    memcpy(b->cam, cam, sizeof(CamT));
}

// make `stream` wait for whatever was last enqueued on the accumulator; afterwards `mark` records the new end
int wait_for(rtw_accum *a, hipStream_t stream) { HIP_TRY(hipStreamWaitEvent(stream, a->ev, 0)); return 0; }
int mark(rtw_accum *a, hipStream_t stream) { HIP_TRY(hipEventRecord(a->ev, stream)); return 0; }

int create(int device, int32_t width, int32_t height, const unsigned long long *host_words, rtw_accum_handle *out) {
    int dev;
    if (int rc = resolve_device(device, &dev)) return rc;
    HIP_TRY(hipSetDevice(dev));
    std::unique_ptr<rtw_accum> a(new rtw_accum());
    memset(&a->bind, 0, sizeof a->bind);
    a->device = dev; a->width = width; a->height = height;
    const size_t bytes = n_pixels(a.get()) * 64u;
    HIP_TRY(hipMalloc((void **)&a->words, bytes));
    hipError_t e = hipEventCreateWithFlags(&a->ev, hipEventDisableTiming);
    if (e == hipSuccess) e = host_words ? hipMemcpy(a->words, host_words, bytes, hipMemcpyHostToDevice) : hipMemset(a->words, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();       // (the null stream's memset: nothing on a non-blocking stream may overtake it)
    if (e == hipSuccess) e = hipEventRecord(a->ev, nullptr);
    if (e != hipSuccess) {
        HIP_IGNORE(hipFree(a->words));
        if (a->ev) HIP_IGNORE(hipEventDestroy(a->ev));
        return fail((int)e, "accumulator of %d x %d: %s", width, height, hipGetErrorString(e));
    }
    *out = a.release();
    return 0;
}

int check_size(int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return fail(-2, "width/height must be positive (got %d x %d)", width, height);
    if ((long long)width * height > (1ll << 28)) return fail(-5, "accumulator too large: %d x %d pixels", width, height);
    return 0;
}

// blocking read of the device words, behind everything enqueued on the accumulator
int read_words(rtw_accum *a, void *host) {
    HIP_TRY(hipSetDevice(a->device));
    HIP_TRY(hipEventSynchronize(a->ev));
    HIP_TRY(hipMemcpy(host, a->words, n_pixels(a) * 64u, hipMemcpyDeviceToHost));
    return 0;
}

template <typename T>
int resolve_dev(rtw_accum *a, int32_t gamma, void *d_out, hipStream_t stream) {
    const long long s = samples_done(a);
    if (s < 1) return fail(-2, "the accumulator holds no samples: nothing to resolve");
    if (a->bind.is_f64 != (sizeof(T) == 8)) return fail(-4, "accumulator precision does not match the call");
    HIP_TRY(hipSetDevice(a->device));
    if (int rc = wait_for(a, stream)) return rc;
    (void)hipGetLastError();
    if (a->adaptive) launch_resolve_tiles<T>(stream, a->words, (T *)d_out, a->d_tiles, (int)a->width, (int)a->height, (int)a->bind.spp, (int)a->bind.chunk_spp, (int)gamma);
    else launch_resolve<T>(stream, a->words, (T *)d_out, (int)a->width, (int)a->height, (int)s, (int)gamma);
    HIP_TRY(hipGetLastError());
    return mark(a, stream);
}

template <typename T>
int resolve_host(rtw_accum *a, int32_t gamma, T *out) {
    if (!a || !out) return fail(-1, "null argument");
    DeviceGuard guard;
    HIP_TRY(hipSetDevice(a->device));
    const size_t bytes = n_pixels(a) * 3u * sizeof(T);
    void *d = nullptr;
    HIP_TRY(hipMalloc(&d, bytes));
    int rc = resolve_dev<T>(a, gamma, d, nullptr);
    if (!rc) { hipError_t e = hipEventSynchronize(a->ev); if (e == hipSuccess) e = hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost); if (e != hipSuccess) rc = fail((int)e, "resolve: %s", hipGetErrorString(e)); }
    HIP_IGNORE(hipFree(d));
    return rc;
}

// Everything about a pass that is decided without a device, in the header's order: nulls, the render's own checks, whole frames on one
// device, the chunk range; then the handles (precision, size, device), the binding, the overlap.  On success *nch / *cs: the effective chunks.
// (validate_frame: the render's own checks and whole frames on one device; validate_handles: precision, size, device)
int validate_frame(const rtw_params *p, int *nch_out, int *cs_out) {
    int nch, cs;
    if (int rc = validate_params(p, &nch, &cs)) return rc;
    if (p->shard_count != 1) return fail(-2, "a progressive render renders whole frames (shard_count = %d)", p->shard_count);
    if (p->flags & RTW_FLAG_COMPACT_TILES) return fail(-2, "a progressive render accumulates whole frames (RTW_FLAG_COMPACT_TILES is a per-shard layout)");
    if (p->flags & RTW_FLAG_RCCL_REDUCE) return fail(-2, "a progressive render runs on one device (RTW_FLAG_RCCL_REDUCE)");
    if (p->flags & RTW_FLAG_RAY_POOL) return fail(-2, "a progressive render runs the lane-loop kernel (RTW_FLAG_RAY_POOL)");
    if (p->n_devices > 1 || p->n_devices < 0 || p->device_ids)
        return fail(-2, "a progressive render runs on one device (n_devices = %d%s)", p->n_devices, p->device_ids ? ", device_ids given" : "");
    *nch_out = nch; *cs_out = cs;
    return 0;
}
int validate_handles(bool call_f64, rtw_scene_handle scene, const rtw_params *p, rtw_accum_handle a) {
    if (scene->is_f64 != call_f64) return fail(-4, "scene handle precision does not match the call");
    if (a->width != p->width || a->height != p->height)
        return fail(-4, "the accumulator is %d x %d, the render %d x %d", a->width, a->height, p->width, p->height);
    if (a->device != scene->device) return fail(-4, "accumulator on device %d, scene on device %d", a->device, scene->device);
    if (p->device >= 0 && p->device != scene->device) return fail(-4, "params.device %d != scene device %d", p->device, scene->device);
    return 0;
}
template <typename CamT>
int validate_accum(rtw_scene_handle scene, const CamT *cam, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, rtw_accum_handle a, int *nch_out, int *cs_out) {
    if (!p) return fail(-1, "null params");
    if (!cam || !a || !scene) return fail(-1, "null argument");
    int nch, cs;
    if (int rc = validate_frame(p, &nch, &cs)) return rc;
    if (int rc = check_chunk_range(chunk_begin, chunk_count, nch)) return rc;
    if (int rc = validate_handles(sizeof(CamT) == sizeof(rtw_camera_f64), scene, p, a)) return rc;
    if (a->adaptive) return fail(-2, "the accumulator is adaptive (its tiles hold different chunk counts): rtw_render_adaptive_* continues it, rtw_accum_reset() makes it a plain one");
    if (a->bound) {
        AccumBind b;
        make_bind(&b, scene, cam, p, nch, cs);
        if (!same_render(a->bind, b)) return fail(-4, "the accumulator is bound to another render (size, precision, seed, spp, chunks, depth, numerics, camera or scene differ); rtw_accum_reset() unbinds it");
        if (overlaps(a->ranges, chunk_begin, chunk_begin + chunk_count))
            return fail(-2, "chunk range [%d, %d) overlaps chunks the accumulator already holds", chunk_begin, chunk_begin + chunk_count);
    }
    *nch_out = nch; *cs_out = cs;
    return 0;
}

// One pass after its validation, for the n_views >= 1 accumulators of a call (`binds`: what each is, or will be, bound to): wait for their
// events, launch, bind, add the range, mark.  `single`: the call came in through rtw_render_accum_* -- the one view's words and divisor
// travel in the pass itself and the non-BATCH instance runs; otherwise the view array and the BATCH instance.
template <typename CamT>
int accum_pass(bool single, rtw_scene_handle scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count,
               const rtw_accum_handle *accums, const AccumBind *binds, void *d_out, void *stream_v) {
    DeviceGuard guard;
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_TRY(hipSetDevice(scene->device));
    std::vector<AccumViewPass> views((size_t)n_views);
    for (int32_t v = 0; v < n_views; ++v) {
        if (int rc = wait_for(accums[v], stream)) return rc;
        views[(size_t)v].words = accums[v]->words;
        views[(size_t)v].samples = (int)(samples_done(accums[v]) + samples_in(binds[v], chunk_begin, (long long)chunk_begin + chunk_count));
    }
    AccumPass pass;
    pass.words = single ? views[0].words : nullptr; pass.chunk_begin = chunk_begin; pass.chunk_count = chunk_count; pass.samples = single ? views[0].samples : 1;
    pass.views = single ? nullptr : views.data();
    RenderRec *rec = nullptr;
    CtxPtr ctx;
    release_last();
    int rc = launch_render<CamElem<CamT>>(scene, cams, single ? 0 : n_views, seeds, p, d_out, stream, &rec, &ctx, &pass);
    hold_last(rec, ctx);               // (also on a late error: released by the next call)
    if (rc) return rc;
    for (int32_t v = 0; v < n_views; ++v) {
        rtw_accum *a = accums[v];
        a->bind = binds[v]; a->bound = true;
        add_range(a->ranges, chunk_begin, chunk_begin + chunk_count);
        if (int rc2 = mark(a, stream)) return rc2;
    }
    return 0;
}

template <typename CamT>
int render_accum(rtw_scene_handle scene, const CamT *cam, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, rtw_accum_handle a, void *d_out, void *stream_v) {
    int nch, cs;
    if (int rc = validate_accum(scene, cam, p, chunk_begin, chunk_count, a, &nch, &cs)) return rc;
    AccumBind b;
    make_bind(&b, scene, cam, p, nch, cs);
    return accum_pass(true, scene, cam, 1, nullptr, p, chunk_begin, chunk_count, &a, &b, d_out, stream_v);
}

// ---- adaptive render ----
int n_tiles_of(const rtw_accum *a) { return tiles_of(a->width, a->height); }
int default_check_chunks(int nch) { int m = std::max(16, (nch + 7) / 8); return m + (m & 1); }      // the smallest even number >= max(16, N / 8)

// everything about an adaptive call that is decided without a device: nulls, the render, whole frames on one device, the adaptive
// parameters; then the handles and the binding.  *eff: the parameters with min_chunks / check_chunks as their effective values.
int validate_adaptive_params(const rtw_adaptive_t *ad, int nch, rtw_adaptive_t *eff) {
    if (!std::isfinite(ad->tolerance) || !(ad->tolerance > 0.0)) return fail(-2, "tolerance must be finite and > 0 (got %g)", ad->tolerance);
    if (!std::isfinite(ad->dark_floor) || ad->dark_floor < 0.0) return fail(-2, "dark_floor must be finite and >= 0 (got %g)", ad->dark_floor);
    if (ad->min_chunks < 0 || (ad->min_chunks & 1)) return fail(-2, "min_chunks must be even and >= 2, or 0 for the default (got %d)", ad->min_chunks);
    if (ad->check_chunks < 0 || (ad->check_chunks & 1)) return fail(-2, "check_chunks must be even and >= 2, or 0 for the default (got %d)", ad->check_chunks);
    memset(eff, 0, sizeof *eff);
    eff->tolerance = ad->tolerance; eff->dark_floor = ad->dark_floor;
    eff->min_chunks = ad->min_chunks ? ad->min_chunks : default_check_chunks(nch);
    eff->check_chunks = ad->check_chunks ? ad->check_chunks : default_check_chunks(nch);
    return 0;
}
template <typename CamT>
int validate_adaptive(rtw_scene_handle scene, const CamT *cam, const rtw_params *p, const rtw_adaptive_t *ad, rtw_accum_handle a, int *nch_out, int *cs_out, rtw_adaptive_t *eff) {
    if (!p) return fail(-1, "null params");
    if (!cam || !a || !scene || !ad) return fail(-1, "null argument");
    int nch, cs;
    if (int rc = validate_frame(p, &nch, &cs)) return rc;
    if (int rc = validate_adaptive_params(ad, nch, eff)) return rc;
    if (int rc = validate_handles(sizeof(CamT) == sizeof(rtw_camera_f64), scene, p, a)) return rc;
    if (a->bound) {
        if (!a->adaptive) return fail(-4, "the accumulator is bound by plain passes (rtw_render_accum_* / merge / import); rtw_accum_reset() unbinds it");
        AccumBind b;
        make_bind(&b, scene, cam, p, nch, cs);
        if (!same_render(a->bind, b)) return fail(-4, "the accumulator is bound to another render (size, precision, seed, spp, chunks, depth, numerics, camera or scene differ); rtw_accum_reset() unbinds it");
        if (a->ad.dark_floor != eff->dark_floor || a->ad.min_chunks != eff->min_chunks || a->ad.check_chunks != eff->check_chunks)
            return fail(-4, "the accumulator's adaptive render has dark_floor %g, min_chunks %d, check_chunks %d: a refinement keeps them", a->ad.dark_floor, a->ad.min_chunks, a->ad.check_chunks);
        if (eff->tolerance > a->ad.tolerance)
            return fail(-4, "tolerance %g is looser than the accumulator's last (%g): refinement only tightens", eff->tolerance, a->ad.tolerance);
    }
    *nch_out = nch; *cs_out = cs;
    return 0;
}

// The loop, after the validation, for the n_views >= 1 accumulators of a call: [0, min_chunks) on all tiles, then per checkpoint c: check
// the tiles that hold exactly c chunks, list the ones not converged, read the list's length back (the round's one host wait), render
// [c, c + check_chunks) for the list.  A refinement walks the same checkpoints: a tile that stopped at c under the looser tolerance is
// looked at again at c, where a fresh run would have decided it.  For a batch that is ONE check over the N * n_tiles tiles, ONE compaction
// into the sorted list of batch-global tiles, ONE read-back and ONE pass over the list per checkpoint; a tile's history does not depend on
// its neighbours', so every view ends with the words and C_t of its own single call.  A view's `rounds` -- the passes that held one of ITS
// tiles -- follows on the host from C_t before and after: a pass at checkpoint c held tile t iff old C_t <= c < new C_t (a fresh run's
// first pass: c = 0); every pass of a single call holds one of its tiles, so there it is the number of passes.
// `single`: the call came in through rtw_render_adaptive_*.  It decides the three launch sites of a round and nothing else: the check
// (accum_tile_check_kernel on the accumulator's own flags / list / count in d_tiles, or accum_tile_check_batch_kernel on the call's
// scratch and view table), the compaction (one workgroup's loop, or count / scan / scatter) and the pass (the ACCUM && ADAPT instance
// with accum_tile_advance_kernel, or the BATCH one with accum_tile_advance_batch_kernel) -- a batch of one view runs the BATCH kernels.
template <typename CamT>
int adaptive_loop(bool single, rtw_scene_handle scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_adaptive_t &eff, int nch, int cs,
                  const rtw_accum_handle *accums, const AccumBind *binds, void *d_out, void *stream_v) {
    using T = typename std::conditional<sizeof(CamT) == sizeof(rtw_camera_f64), double, float>::type;
    DeviceGuard guard;
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_TRY(hipSetDevice(scene->device));
    rtw_accum *a0 = accums[0];
    const int n_tiles = n_tiles_of(a0);
    const long long n_all = (long long)n_views * n_tiles;            // (validate_batch: fits an int with room to spare)
    const bool fresh = !a0->bound;
    // (from here on a HIP failure can leave an unbound accumulator with its tile array allocated and cleared: nothing a caller can see --
    //  words, binding and ranges are touched only behind a pass that was launched -- and what the next adaptive call expects to find or make)
    for (int32_t v = 0; v < n_views; ++v) {
        rtw_accum *a = accums[v];
        if (!a->d_tiles) HIP_TRY(hipMalloc((void **)&a->d_tiles, ((size_t)n_tiles * 3u + 4u) * sizeof(int32_t)));
        if (int rc = wait_for(a, stream)) return rc;
        if (fresh) HIP_TRY(hipMemsetAsync(a->d_tiles, 0, (size_t)n_tiles * sizeof(int32_t), stream));
        else if (!a->ad_complete || a->tile_chunks.size() != (size_t)n_tiles) {      // (after a call that failed half way: what the device holds)
            a->tile_chunks.resize((size_t)n_tiles);
            HIP_TRY(hipMemcpyAsync(a->tile_chunks.data(), a->d_tiles, (size_t)n_tiles * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
    }
    // flags | list | count: the single call's lie behind C_t in its accumulator's d_tiles; a batch's in the call's scratch, made once:
    // the views' table | flags | list | count | the compaction's block offsets
    struct Scratch { void *p = nullptr; ~Scratch() { if (p) HIP_IGNORE(hipFree(p)); } } scratch;
    const size_t tab_bytes = ((size_t)n_views * sizeof(TileView) + 15u) / 16u * 16u;
    const int n_blocks = compact_blocks(n_all);
    if (!single) HIP_TRY(hipMalloc(&scratch.p, tab_bytes + ((size_t)n_all * 2u + 4u + (size_t)n_blocks) * sizeof(int32_t)));
    TileView *d_views = static_cast<TileView *>(scratch.p);
    int32_t *d_flags = single ? a0->d_tiles + n_tiles : reinterpret_cast<int32_t *>(static_cast<char *>(scratch.p) + tab_bytes);
    int32_t *d_list = d_flags + n_all, *d_count = d_list + n_all, *d_blocks = d_count + 4;
    // (measurement aid: RTW_BATCH_COMPACT=loop makes a batch's list with the single call's one-workgroup loop -- the same list)
    static const bool compact_loop = aid_env("RTW_BATCH_COMPACT") != nullptr && strcmp(aid_env("RTW_BATCH_COMPACT"), "loop") == 0;
    std::vector<TileView> h_views((size_t)n_views);
    std::vector<AccumViewPass> views((size_t)n_views);
    std::vector<std::vector<int32_t>> old_chunks((size_t)n_views);
    bool settled = !fresh;                   // (the same tolerance again: nothing to decide)
    int later_max = 0;                       // refinement: the last checkpoint some tile of some view stopped at
    for (int32_t v = 0; v < n_views; ++v) {
        rtw_accum *a = accums[v];
        h_views[(size_t)v] = TileView{a->words, a->d_tiles};
        views[(size_t)v] = AccumViewPass{a->words, 1};                // (no running image: the divisor is unused)
        old_chunks[(size_t)v] = fresh ? std::vector<int32_t>((size_t)n_tiles, 0) : a->tile_chunks;
        if (!fresh) for (int32_t c : a->tile_chunks) if (c < nch) later_max = std::max(later_max, (int)c);
        settled = settled && a->ad_complete && eff.tolerance == a->ad.tolerance;
    }
    if (!single) HIP_TRY(hipMemcpyAsync(d_views, h_views.data(), (size_t)n_views * sizeof(TileView), hipMemcpyHostToDevice, stream));    // (h_views outlives the call's last synchronisation)

    release_last();
    rtw_stats_t agg;
    memset(&agg, 0, sizeof agg);
    RenderRec *rec = nullptr;
    CtxPtr ctx;
    std::vector<int> pass_at;                // the checkpoints of this call's passes (0: a fresh run's first)
    // one pass: launch, C_t += count; the caller synchronises the stream before `finish` reads the pass's counters
    auto pass = [&](int begin, int count, const int32_t *list, int n_list) -> int {
        AccumPass ps;
        ps.words = single ? a0->words : nullptr; ps.chunk_begin = begin; ps.chunk_count = count; ps.samples = 1;
        ps.adapt = true; ps.tile_list = list; ps.list_tiles = n_list; ps.views = single ? nullptr : views.data();
        int rc = launch_render<CamElem<CamT>>(scene, cams, single ? 0 : n_views, seeds, p, nullptr, stream, &rec, &ctx, &ps);
        if (rc) { hold_last(rec, ctx); rec = nullptr; return rc; }     // (released by the next call)
        (void)hipGetLastError();
        if (single) launch_tile_advance(stream, list, n_list, a0->d_tiles, count);
        else launch_tile_advance_batch(stream, list, n_list, d_views, n_tiles, count);
        HIP_TRY(hipGetLastError());
        pass_at.push_back(begin);
        return 0;
    };
    auto finish = [&]() -> int {              // (behind a stream synchronisation) the last pass's counters -> agg; its record goes back to the pool
        if (!rec) return 0;
        rtw_stats_t one;
        memset(&one, 0, sizeof one);
        int rc = resolve_rec(rec, &one);
        release_rec(ctx, rec, rc == 0);
        rec = nullptr;
        if (rc) return rc;
        agg.samples += one.samples; agg.segments += one.segments; agg.sphere_tests += one.sphere_tests;
        agg.kernel_ms += one.kernel_ms; agg.total_ms += one.total_ms;
        agg.grid_blocks = std::max(agg.grid_blocks, one.grid_blocks); agg.block_threads = std::max(agg.block_threads, one.block_threads);
        return 0;
    };
    auto run = [&]() -> int {
        const int first = std::min((int)eff.min_chunks, nch);
        long long moved = 0;                    // tiles the last pass brought to the checkpoint at hand
        if (fresh) {
            if (int rc = pass(0, first, nullptr, (int)n_all)) return rc;
            for (int32_t v = 0; v < n_views; ++v) { rtw_accum *a = accums[v]; a->bind = binds[v]; a->bound = true; a->adaptive = true; a->ad = eff; }
            moved = n_all;
        }
        for (int32_t v = 0; v < n_views; ++v) { accums[v]->ad.tolerance = eff.tolerance; accums[v]->ad_complete = false; }
        for (int c = first; c < nch && !settled; c += eff.check_chunks) {
            if (moved == 0 && c > later_max) break;
            (void)hipGetLastError();
            if (single) launch_tile_check(stream, a0->words, a0->d_tiles, d_flags, (int)a0->width, (int)a0->height, c, cs, eff.tolerance, eff.dark_floor);
            else launch_tile_check_batch(stream, d_views, d_flags, (int)n_views, (int)a0->width, (int)a0->height, c, cs, eff.tolerance, eff.dark_floor);
            if (single || compact_loop) launch_compact_loop(stream, d_flags, d_list, d_count, (int)n_all);
            else launch_compact_blocks(stream, d_flags, d_blocks, d_list, d_count, (int)n_all);
            HIP_TRY(hipGetLastError());
            int32_t n_active = 0;
            HIP_TRY(hipMemcpyAsync(&n_active, d_count, sizeof n_active, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (int rc = finish()) return rc;
            if (n_active < 0 || n_active > n_all) return fail(-3, "adaptive render: %d active tiles of %lld", n_active, n_all);
            moved = n_active;
            if (n_active == 0) continue;
            if (int rc = pass(c, std::min((int)eff.check_chunks, nch - c), d_list, n_active)) return rc;
        }
        for (int32_t v = 0; v < n_views; ++v) {
            rtw_accum *a = accums[v];
            a->tile_chunks.resize((size_t)n_tiles);
            HIP_TRY(hipMemcpyAsync(a->tile_chunks.data(), a->d_tiles, (size_t)n_tiles * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        }
        HIP_TRY(hipStreamSynchronize(stream));
        if (int rc = finish()) return rc;
        for (int32_t v = 0; v < n_views; ++v) {
            rtw_accum *a = accums[v];
            const std::vector<int32_t> &was = old_chunks[(size_t)v];
            int min_c = nch, rounds = 0;
            for (int32_t c : a->tile_chunks) min_c = std::min(min_c, (int)c);
            for (int at : pass_at) {
                bool held = false;
                for (int t = 0; t < n_tiles && !held; ++t) held = was[(size_t)t] <= at && at < a->tile_chunks[(size_t)t];
                rounds += held ? 1 : 0;
            }
            a->ranges.clear();
            a->ranges.emplace_back(0, min_c);
            a->ad_complete = true;
            a->ad_rounds = rounds;
            if (d_out)
                if (int rc = resolve_dev<T>(a, p->gamma, static_cast<T *>(d_out) + (size_t)v * n_pixels(a) * 3u, stream)) return rc;
        }
        if (d_out) HIP_TRY(hipStreamSynchronize(stream));
        return 0;
    };
    const int rc = run();
    hold_last(rec, ctx);               // (a failure between a pass and its wait)
    if (rc) {
        for (int32_t v = 0; v < n_views; ++v) if (accums[v]->bound) HIP_IGNORE(hipEventRecord(accums[v]->ev, stream));
        if (scratch.p) HIP_IGNORE(hipStreamSynchronize(stream));               // (the scratch is freed on return)
        return rc;
    }
    agg.n_chunks = nch;
    g_last.agg = agg;
    g_last.resolved = true;
    g_last.per_device.emplace_back(scene->device, agg.kernel_ms);
    for (int32_t v = 0; v < n_views; ++v) if (int rc2 = mark(accums[v], stream)) return rc2;
    return 0;
}

template <typename CamT>
int render_adaptive(rtw_scene_handle scene, const CamT *cam, const rtw_params *p, const rtw_adaptive_t *ad, rtw_accum_handle a, void *d_out, void *stream_v) {
    int nch, cs;
    rtw_adaptive_t eff;
    if (int rc = validate_adaptive(scene, cam, p, ad, a, &nch, &cs, &eff)) return rc;
    AccumBind b;
    make_bind(&b, scene, cam, p, nch, cs);
    return adaptive_loop(true, scene, cam, 1, nullptr, p, eff, nch, cs, &a, &b, d_out, stream_v);
}

// ---- batched passes (rtw_render_accum_batch_*, rtw_render_adaptive_batch_*): N views of one scene, each with its own accumulator ----
// what both batched calls decide before they look at a handle: nulls, n_views, the frame (validate_frame), the queue limit of a batch
int validate_views(rtw_scene_handle scene, const void *cams, int32_t n_views, const rtw_params *p, const rtw_accum_handle *accums, int *nch_out, int *cs_out) {
    if (!p) return fail(-1, "null params");
    if (!cams || !accums || !scene) return fail(-1, "null argument");
    if (n_views < 1) return fail(-2, "n_views must be >= 1 (got %d)", n_views);
    for (int32_t v = 0; v < n_views; ++v) if (!accums[v]) return fail(-1, "null accumulator (view %d)", v);
    if (int rc = validate_frame(p, nch_out, cs_out)) return rc;
    return validate_batch(cams, n_views, p, cams);       // (what is left of it: -5 for a batch whose jobs the queues cannot number)
}
int validate_distinct(int32_t n_views, const rtw_accum_handle *accums) {
    std::vector<rtw_accum_handle> sorted(accums, accums + n_views);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(-2, "one accumulator is given for two views");
    return 0;
}
rtw_params view_params(const rtw_params *p, const uint64_t *seeds, int v) { rtw_params q = *p; if (seeds) q.seed = seeds[v]; return q; }

template <typename CamT>
int render_accum_batch(rtw_scene_handle scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count,
                       const rtw_accum_handle *accums, void *d_out, void *stream_v) {
    int nch, cs;
    if (int rc = validate_views(scene, cams, n_views, p, accums, &nch, &cs)) return rc;
    if (int rc = check_chunk_range(chunk_begin, chunk_count, nch)) return rc;
    if (int rc = validate_distinct(n_views, accums)) return rc;
    // every accumulator on its own, as rtw_render_accum_* validates it -- all of them before anything is touched
    std::vector<AccumBind> binds((size_t)n_views);
    for (int32_t v = 0; v < n_views; ++v) {
        const rtw_params q = view_params(p, seeds, v);
        int nv, cv;
        if (int rc = validate_accum(scene, cams + v, &q, chunk_begin, chunk_count, accums[v], &nv, &cv)) return fail(rc, "view %d: %s", v, std::string(g_err).c_str());
        make_bind(&binds[(size_t)v], scene, cams + v, &q, nch, cs);
    }
    return accum_pass(false, scene, cams, n_views, seeds, p, chunk_begin, chunk_count, accums, binds.data(), d_out, stream_v);
}

template <typename CamT>
int render_adaptive_batch(rtw_scene_handle scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_adaptive_t *ad,
                          const rtw_accum_handle *accums, void *d_out, void *stream_v) {
    if (!p) return fail(-1, "null params");
    if (!ad) return fail(-1, "null argument");
    int nch, cs;
    if (int rc = validate_views(scene, cams, n_views, p, accums, &nch, &cs)) return rc;
    rtw_adaptive_t eff;
    if (int rc = validate_adaptive_params(ad, nch, &eff)) return rc;
    if (int rc = validate_distinct(n_views, accums)) return rc;
    std::vector<AccumBind> binds((size_t)n_views);
    // (a mixed array is refused at its first view that fails either test, so WHICH -4 message it gets -- "bound by plain passes", "another
    //  render", "all unbound or all adaptive" -- depends on the order of the views; the code does not)
    for (int32_t v = 0; v < n_views; ++v) {          // every accumulator on its own, as rtw_render_adaptive_* validates it -- all before anything is touched
        const rtw_params q = view_params(p, seeds, v);
        int nv, cv;
        if (int rc = validate_adaptive(scene, cams + v, &q, ad, accums[v], &nv, &cv, &eff)) return fail(rc, "view %d: %s", v, std::string(g_err).c_str());
        make_bind(&binds[(size_t)v], scene, cams + v, &q, nch, cs);
        if (accums[v]->bound != accums[0]->bound) return fail(-4, "view %d: the accumulators of a batch are all unbound or all adaptive accumulators of their views' renders", v);
    }
    return adaptive_loop(false, scene, cams, n_views, seeds, p, eff, nch, cs, accums, binds.data(), d_out, stream_v);
}

int adaptive_info(const rtw_accum *a, rtw_adaptive_info_t *out) {
    memset(out, 0, sizeof *out);
    const int tiles_i = (a->height + 7) / 8, tiles_j = (a->width + 7) / 8, nch = a->bind.n_chunks;
    out->n_tiles = tiles_i * tiles_j; out->rounds = a->ad_rounds; out->tolerance = a->ad.tolerance;
    out->min_chunks_held = nch; out->max_chunks_held = 0;
    for (int tj = 0; tj < tiles_j; ++tj)
        for (int ti = 0; ti < tiles_i; ++ti) {
            const int c = a->tile_chunks[(size_t)tj * (size_t)tiles_i + (size_t)ti];
            const long long npix = (long long)std::min(8, a->height - 8 * ti) * std::min(8, a->width - 8 * tj);
            out->samples += (uint64_t)(npix * samples_in(a->bind, 0, c));
            if (c < nch) ++out->tiles_converged; else ++out->tiles_at_cap;
            out->min_chunks_held = std::min(out->min_chunks_held, c); out->max_chunks_held = std::max(out->max_chunks_held, c);
        }
    return 0;
}

// ---- an accumulator as the denoiser's input (include/rtw_hip.h rtw_accum_features_*, rtw_accum_noise_*): everything here READS the words and
// C_t; the calls wait for the accumulator's event and record it afterwards, so a later pass cannot overwrite them under a running kernel ----
// an adaptive accumulator whose last call finished: C_t on the device is what the host copy says
int check_adaptive_complete(const rtw_accum *a) {
    if (!a->ad_complete || !a->d_tiles || a->tile_chunks.size() != (size_t)n_tiles_of(a))
        return fail(-2, "the accumulator's last adaptive call did not finish: its tiles' chunk counts are not settled");
    return 0;
}
}  // namespace
// (validate_ / enqueue_accum_features: declared in rtw_host.hpp, rtw_accum_filtered_* runs them too)
template <typename CamT>
int validate_accum_features(rtw_scene_handle scene, const CamT *cam, const rtw_params *p, rtw_accum_handle a) {
    if (!p) return fail(-1, "null params");
    if (!cam || !a || !scene) return fail(-1, "null argument");
    int nch, cs;
    if (int rc = validate_features(p, 0, 1, &nch, &cs)) return rc;
    if (int rc = validate_handles(sizeof(CamT) == sizeof(rtw_camera_f64), scene, p, a)) return rc;
    if (!a->bound) return fail(-2, "the accumulator holds no chunk interval: there is nothing to take features of");
    AccumBind b;
    make_bind(&b, scene, cam, p, nch, cs);
    if (!same_render(a->bind, b)) return fail(-4, "the accumulator is bound to another render (size, precision, seed, spp, chunks, depth, numerics, camera or scene differ)");
    if (a->adaptive) return check_adaptive_complete(a);
    if (a->ranges.size() != 1) return fail(-2, "the accumulator holds %d chunk intervals: a feature pass covers exactly one", (int)a->ranges.size());
    return 0;
}
template <typename CamT>
int enqueue_accum_features(rtw_scene_handle scene, const CamT *cam, const rtw_params *p, rtw_accum_handle a, void *d_out, hipStream_t stream, RenderRec **rec, CtxPtr *ctx) {
    HIP_TRY(hipSetDevice(a->device));
    if (int rc = wait_for(a, stream)) return rc;
    int rc;
    if (a->adaptive) rc = launch_features<CamElem<CamT>>(scene, cam, 0, nullptr, p, 0, 1, d_out, stream, rec, ctx, a->d_tiles);
    else rc = launch_features<CamElem<CamT>>(scene, cam, 0, nullptr, p, a->ranges[0].first, a->ranges[0].second - a->ranges[0].first, d_out, stream, rec, ctx);
    if (rc) return rc;
    return mark(a, stream);
}
template int validate_accum_features(rtw_scene_handle, const rtw_camera_f32 *, const rtw_params *, rtw_accum_handle);
template int validate_accum_features(rtw_scene_handle, const rtw_camera_f64 *, const rtw_params *, rtw_accum_handle);
template int enqueue_accum_features(rtw_scene_handle, const rtw_camera_f32 *, const rtw_params *, rtw_accum_handle, void *, hipStream_t, RenderRec **, CtxPtr *);
template int enqueue_accum_features(rtw_scene_handle, const rtw_camera_f64 *, const rtw_params *, rtw_accum_handle, void *, hipStream_t, RenderRec **, CtxPtr *);
namespace {
template <typename CamT>
int accum_features(rtw_scene_handle scene, const CamT *cam, const rtw_params *p, rtw_accum_handle a, void *d_out, void *stream_v) {
    // (nulls, the render's own checks and the buffer before a handle is looked at, like the device form of the feature pass)
    if (!p) return fail(-1, "null params");
    if (!cam || !a || !scene || !d_out) return fail(-1, "null argument");
    int nch, cs;
    if (int rc = validate_features(p, 0, 1, &nch, &cs)) return rc;
    if (((uintptr_t)d_out & 15u) != 0) return fail(-2, "the feature buffer must be 16-byte aligned");
    if (int rc = validate_accum_features(scene, cam, p, a)) return rc;
    DeviceGuard guard;
    RenderRec *rec = nullptr;
    CtxPtr ctx;
    release_last();
    const int rc = enqueue_accum_features(scene, cam, p, a, d_out, (hipStream_t)stream_v, &rec, &ctx);
    hold_last(rec, ctx);               // (also on a late error: released by the next call)
    return rc;
}

// ---- the same for a batch (rtw_accum_resolve_batch_*, rtw_accum_features_batch_*, rtw_accum_noise_batch_*): N accumulators of one size on one
// device, ONE launch per pass; every call waits for EVERY accumulator's event and records it on every one afterwards ----
// (validate_accum_array, rtw_host.hpp: a null array or entry, the count -- every batched entry point calls it once, before anything looks at an entry)
// accumulators of ONE size on ONE device: what the one launch's geometry and the one output buffer need
int validate_same_frame(const rtw_accum_handle *accums, int32_t n_views) {
    const rtw_accum *a0 = accums[0];
    for (int32_t v = 1; v < n_views; ++v) {
        const rtw_accum *a = accums[v];
        if (a->width != a0->width || a->height != a0->height) return fail(-4, "view %d: the accumulator is %d x %d, view 0's %d x %d", v, a->width, a->height, a0->width, a0->height);
        if (a->device != a0->device) return fail(-4, "view %d: accumulator on device %d, view 0's on device %d", v, a->device, a0->device);
    }
    return 0;
}
int wait_for_all(const rtw_accum_handle *accums, int32_t n_views, hipStream_t stream) {
    for (int32_t v = 0; v < n_views; ++v) if (int rc = wait_for(accums[v], stream)) return rc;
    return 0;
}
int mark_all(const rtw_accum_handle *accums, int32_t n_views, hipStream_t stream) {
    for (int32_t v = 0; v < n_views; ++v) if (int rc = mark(accums[v], stream)) return rc;
    return 0;
}
// The views' table {words, C_t or null, divisor, spp, chunk size} on the device, by ONE H2D on `stream` (which already waits for the accumulators'
// events).  It lives with the FIRST accumulator: whatever read the table before is ordered in front of that accumulator's event, hence in
// front of this copy.  A call whose table is the one the device already holds -- the resolve and the noise map of one batch, a turntable
// read again -- uploads nothing and does not wait; only a DIFFERENT table waits on the host until the previous copy has left the pinned
// staging buffer (tab_ev).  (forget_views: after a failure behind the copy the device table counts as unknown.)
void forget_views(rtw_accum *a0) { a0->tab_bytes = 0; }
int stage_views(const rtw_accum_handle *accums, int32_t n_views, hipStream_t stream, const ReadView **d_views) {
    rtw_accum *a0 = accums[0];
    const size_t bytes = (size_t)n_views * sizeof(ReadView);
    std::vector<ReadView> tab((size_t)n_views);
    for (int32_t v = 0; v < n_views; ++v) {
        const rtw_accum *a = accums[v];
        tab[(size_t)v] = ReadView{a->words, a->adaptive ? a->d_tiles : nullptr, (int)samples_done(a), (int)a->bind.spp, (int)a->bind.chunk_spp, 0};
    }
    *d_views = static_cast<const ReadView *>(a0->d_tab);
    if (a0->tab_bytes == bytes && memcmp(a0->h_tab, tab.data(), bytes) == 0) return 0;
    forget_views(a0);
    if (a0->tab_ev) HIP_TRY(hipEventSynchronize(a0->tab_ev));
    else HIP_TRY(hipEventCreateWithFlags(&a0->tab_ev, hipEventDisableTiming));
    if (a0->tab_cap < bytes) {
        if (a0->d_tab) { HIP_IGNORE(hipFree(a0->d_tab)); a0->d_tab = nullptr; }            // (hipFree waits for the device: nothing reads the old table)
        if (a0->h_tab) { HIP_IGNORE(hipHostFree(a0->h_tab)); a0->h_tab = nullptr; }
        a0->tab_cap = 0;
        HIP_TRY(hipMalloc(&a0->d_tab, bytes));
        HIP_TRY(hipHostMalloc(&a0->h_tab, bytes, hipHostMallocDefault));
        a0->tab_cap = bytes;
    }
    memcpy(a0->h_tab, tab.data(), bytes);
    HIP_TRY(hipMemcpyAsync(a0->d_tab, a0->h_tab, bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(a0->tab_ev, stream));
    a0->tab_bytes = bytes;
    *d_views = static_cast<const ReadView *>(a0->d_tab);
    return 0;
}
// what follows the table in both read-only passes: the launch's error, then every accumulator's event; a failure forgets the table
int finish_read_batch(const rtw_accum_handle *accums, int32_t n_views, hipStream_t stream) {
    const hipError_t e = hipGetLastError();
    int rc = e == hipSuccess ? mark_all(accums, n_views, stream) : fail((int)e, "batched pass over %d accumulators: %s", n_views, hipGetErrorString(e));
    if (rc) forget_views(accums[0]);
    return rc;
}

// rtw_accum_resolve_batch_*: what rtw_accum_resolve_* refuses, for every view, and the batch's own rules
int validate_resolve_batch(const rtw_accum_handle *accums, int32_t n_views, bool f64) {
    if (int rc = validate_distinct(n_views, accums)) return rc;
    for (int32_t v = 0; v < n_views; ++v) {
        const rtw_accum *a = accums[v];
        if (samples_done(a) < 1) return fail(-2, "view %d: the accumulator holds no samples: nothing to resolve", v);
        if (a->adaptive) if (int rc = check_adaptive_complete(a)) return fail(rc, "view %d: %s", v, std::string(g_err).c_str());
        if ((a->bind.is_f64 != 0) != f64) return fail(-4, "view %d: accumulator precision does not match the call", v);
    }
    if (int rc = validate_same_frame(accums, n_views)) return rc;
    if ((double)n_pixels(accums[0]) * (double)n_views >= (double)(1ll << 37)) return fail(-5, "batch too large for one call: %d views of %d x %d pixels", n_views, accums[0]->width, accums[0]->height);
    return 0;
}
template <typename T>
int resolve_batch_dev(const rtw_accum_handle *accums, int32_t n_views, int32_t gamma, void *d_out, hipStream_t stream) {
    rtw_accum *a0 = accums[0];
    HIP_TRY(hipSetDevice(a0->device));
    if (int rc = wait_for_all(accums, n_views, stream)) return rc;
    const ReadView *d_views = nullptr;
    if (int rc = stage_views(accums, n_views, stream, &d_views)) return rc;
    (void)hipGetLastError();
    launch_resolve_batch<T>(stream, d_views, (T *)d_out, (int)n_views, (int)a0->width, (int)a0->height, (int)gamma);
    return finish_read_batch(accums, n_views, stream);
}
template <typename T>
int resolve_batch(const rtw_accum_handle *accums, int32_t n_views, int32_t gamma, void *d_out, void *stream_v) {
    if (!d_out) return fail(-1, "null argument");
    if (int rc = validate_accum_array(accums, n_views)) return rc;
    if ((uintptr_t)d_out & (sizeof(T) - 1)) return fail(-2, "the frames must be aligned to their element type");
    if (int rc = validate_resolve_batch(accums, n_views, sizeof(T) == 8)) return rc;
    DeviceGuard guard;
    return resolve_batch_dev<T>(accums, n_views, gamma, d_out, (hipStream_t)stream_v);
}

}  // namespace
// rtw_accum_features_batch_*: the handles of a batched feature pass, after the checks that look at no handle -- every view as
// rtw_accum_features_* validates it (with its own camera and seed), then the batch's rule: all adaptive, or all uniform with ONE interval
template <typename CamT>
int validate_accum_features_batch(rtw_scene_handle scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_accum_handle *accums) {
    if (int rc = validate_distinct(n_views, accums)) return rc;
    for (int32_t v = 0; v < n_views; ++v) {
        const rtw_params q = view_params(p, seeds, v);
        if (int rc = validate_accum_features(scene, cams + v, &q, accums[v])) return fail(rc, "view %d: %s", v, std::string(g_err).c_str());
    }
    const rtw_accum *a0 = accums[0];
    for (int32_t v = 1; v < n_views; ++v) {
        const rtw_accum *a = accums[v];
        if (a->adaptive != a0->adaptive) return fail(-2, "view %d: the accumulators of a batched feature pass are all adaptive or all uniform", v);
        if (!a->adaptive && a->ranges[0] != a0->ranges[0])
            return fail(-2, "view %d holds the chunks [%d, %d), view 0 [%d, %d): uniform accumulators of a batched feature pass hold ONE interval", v, a->ranges[0].first,
                        a->ranges[0].second, a0->ranges[0].first, a0->ranges[0].second);
    }
    return 0;
}
template <typename CamT>
int enqueue_accum_features_batch(rtw_scene_handle scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_accum_handle *accums, void *d_out,
                                 hipStream_t stream, RenderRec **rec, CtxPtr *ctx) {
    const rtw_accum *a0 = accums[0];
    HIP_TRY(hipSetDevice(a0->device));
    if (int rc = wait_for_all(accums, n_views, stream)) return rc;
    int rc;
    if (a0->adaptive) {
        std::vector<const int *> tiles((size_t)n_views);
        for (int32_t v = 0; v < n_views; ++v) tiles[(size_t)v] = accums[v]->d_tiles;
        rc = launch_features<CamElem<CamT>>(scene, cams, n_views, seeds, p, 0, 1, d_out, stream, rec, ctx, nullptr, tiles.data());
    } else rc = launch_features<CamElem<CamT>>(scene, cams, n_views, seeds, p, a0->ranges[0].first, a0->ranges[0].second - a0->ranges[0].first, d_out, stream, rec, ctx);
    if (rc) return rc;
    return mark_all(accums, n_views, stream);
}
template int validate_accum_features_batch(rtw_scene_handle, const rtw_camera_f32 *, int32_t, const uint64_t *, const rtw_params *, const rtw_accum_handle *);
template int validate_accum_features_batch(rtw_scene_handle, const rtw_camera_f64 *, int32_t, const uint64_t *, const rtw_params *, const rtw_accum_handle *);
template int enqueue_accum_features_batch(rtw_scene_handle, const rtw_camera_f32 *, int32_t, const uint64_t *, const rtw_params *, const rtw_accum_handle *, void *, hipStream_t, RenderRec **, CtxPtr *);
template int enqueue_accum_features_batch(rtw_scene_handle, const rtw_camera_f64 *, int32_t, const uint64_t *, const rtw_params *, const rtw_accum_handle *, void *, hipStream_t, RenderRec **, CtxPtr *);
namespace {
template <typename CamT>
int accum_features_batch(rtw_scene_handle scene, const CamT *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_accum_handle *accums, void *d_out, void *stream_v) {
    if (!p) return fail(-1, "null params");
    if (!cams || !accums || !scene || !d_out) return fail(-1, "null argument");
    if (int rc = validate_accum_array(accums, n_views)) return rc;
    int nch, cs;
    if (int rc = validate_features_batch(cams, n_views, p, 0, 1, d_out, &nch, &cs)) return rc;
    if (((uintptr_t)d_out & 15u) != 0) return fail(-2, "the feature buffer must be 16-byte aligned");
    if (int rc = validate_accum_features_batch(scene, cams, n_views, seeds, p, accums)) return rc;
    DeviceGuard guard;
    RenderRec *rec = nullptr;
    CtxPtr ctx;
    release_last();
    const int rc = enqueue_accum_features_batch(scene, cams, n_views, seeds, p, accums, d_out, (hipStream_t)stream_v, &rec, &ctx);
    hold_last(rec, ctx);               // (also on a late error: released by the next call)
    return rc;
}

}  // namespace

// the array of a batched call itself: a null array or entry, the count
int validate_accum_array(const rtw_accum_handle *accums, int32_t n_views) {
    if (!accums) return fail(-1, "null argument");
    if (n_views < 1) return fail(-2, "n_views must be >= 1 (got %d)", n_views);
    for (int32_t v = 0; v < n_views; ++v) if (!accums[v]) return fail(-1, "null accumulator (view %d)", v);
    return 0;
}
int accum_device_of(rtw_accum_handle a) { return a->device; }
bool accum_is_adaptive(rtw_accum_handle a) { return a->adaptive; }
int validate_accum_noise(rtw_accum_handle a, bool f64) {
    if (!a) return fail(-1, "null argument");
    if (!a->adaptive) return fail(-2, "the accumulator is not adaptive: word 7 of its pixels is 0 by contract, it carries no noise measurement");
    if (int rc = check_adaptive_complete(a)) return rc;
    if ((a->bind.is_f64 != 0) != f64) return fail(-4, "accumulator precision does not match the call");
    return 0;
}
int enqueue_accum_noise(rtw_accum_handle a, bool f64, void *d_out, hipStream_t stream) {
    HIP_TRY(hipSetDevice(a->device));
    if (int rc = wait_for(a, stream)) return rc;
    (void)hipGetLastError();
    if (f64) launch_noise<double>(stream, a->words, (double *)d_out, a->d_tiles, (int)a->width, (int)a->height, (int)a->bind.spp, (int)a->bind.chunk_spp, a->ad.dark_floor);
    else launch_noise<float>(stream, a->words, (float *)d_out, a->d_tiles, (int)a->width, (int)a->height, (int)a->bind.spp, (int)a->bind.chunk_spp, a->ad.dark_floor);
    HIP_TRY(hipGetLastError());
    return mark(a, stream);
}
int enqueue_accum_resolve(rtw_accum_handle a, bool f64, int32_t gamma, void *d_out, hipStream_t stream) {
    return f64 ? resolve_dev<double>(a, gamma, d_out, stream) : resolve_dev<float>(a, gamma, d_out, stream);
}
// the batched forms (rtw_accum_filtered_batch_* strings them together as the single call strings the ones above)
// every view as rtw_accum_noise_* validates it; one frame size and device; ONE spp, chunk size and dark_floor -- the kernel takes one set
int validate_accum_noise_batch(const rtw_accum_handle *accums, int32_t n_views, bool f64) {
    if (int rc = validate_distinct(n_views, accums)) return rc;
    for (int32_t v = 0; v < n_views; ++v)
        if (int rc = validate_accum_noise(accums[v], f64)) return fail(rc, "view %d: %s", v, std::string(g_err).c_str());
    if (int rc = validate_same_frame(accums, n_views)) return rc;
    const rtw_accum *a0 = accums[0];
    for (int32_t v = 1; v < n_views; ++v) {
        const rtw_accum *a = accums[v];
        if (a->bind.spp != a0->bind.spp || a->bind.chunk_spp != a0->bind.chunk_spp || a->ad.dark_floor != a0->ad.dark_floor)
            return fail(-4, "view %d: spp %d, chunk size %d, dark_floor %g; view 0: %d, %d, %g -- the noise maps of a batch share them", v, a->bind.spp, a->bind.chunk_spp, a->ad.dark_floor,
                        a0->bind.spp, a0->bind.chunk_spp, a0->ad.dark_floor);
    }
    if ((double)n_pixels(a0) * (double)n_views >= (double)(1ll << 39)) return fail(-5, "batch too large for one call: %d views of %d x %d pixels", n_views, a0->width, a0->height);
    return 0;
}
int enqueue_accum_noise_batch(const rtw_accum_handle *accums, int32_t n_views, bool f64, void *d_out, hipStream_t stream) {
    rtw_accum *a0 = accums[0];
    HIP_TRY(hipSetDevice(a0->device));
    if (int rc = wait_for_all(accums, n_views, stream)) return rc;
    const ReadView *d_views = nullptr;
    if (int rc = stage_views(accums, n_views, stream, &d_views)) return rc;
    (void)hipGetLastError();
    if (f64) launch_noise_batch<double>(stream, d_views, (double *)d_out, (int)n_views, (int)a0->width, (int)a0->height, (int)a0->bind.spp, (int)a0->bind.chunk_spp, a0->ad.dark_floor);
    else launch_noise_batch<float>(stream, d_views, (float *)d_out, (int)n_views, (int)a0->width, (int)a0->height, (int)a0->bind.spp, (int)a0->bind.chunk_spp, a0->ad.dark_floor);
    return finish_read_batch(accums, n_views, stream);
}
int validate_accum_resolve_batch(const rtw_accum_handle *accums, int32_t n_views, bool f64) { return validate_resolve_batch(accums, n_views, f64); }
int enqueue_accum_resolve_batch(const rtw_accum_handle *accums, int32_t n_views, bool f64, int32_t gamma, void *d_out, hipStream_t stream) {
    return f64 ? resolve_batch_dev<double>(accums, n_views, gamma, d_out, stream) : resolve_batch_dev<float>(accums, n_views, gamma, d_out, stream);
}

}  // namespace rtwh

using namespace rtwh;

extern "C" {

int rtw_accum_create(int device, int32_t width, int32_t height, rtw_accum_handle *out) {
    if (!out) return fail(-1, "null argument");
    if (int rc = check_size(width, height)) return rc;
    DeviceGuard guard;
    return create(device, width, height, nullptr, out);
}

int rtw_accum_reset(rtw_accum_handle a, void *stream_v) {
    if (!a) return fail(-1, "null argument");
    DeviceGuard guard;
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_TRY(hipSetDevice(a->device));
    if (int rc = wait_for(a, stream)) return rc;
    HIP_TRY(hipMemsetAsync(a->words, 0, n_pixels(a) * 64u, stream));
    a->bound = false;
    a->ranges.clear();
    memset(&a->bind, 0, sizeof a->bind);
    a->adaptive = false; a->ad_complete = false; a->ad_rounds = 0; a->tile_chunks.clear();      // (the tile counts are zeroed by the next adaptive call)
    memset(&a->ad, 0, sizeof a->ad);
    return mark(a, stream);
}

int rtw_accum_free(rtw_accum_handle a) {
    if (!a) return 0;
    DeviceGuard guard;
    HIP_IGNORE(hipSetDevice(a->device));
    if (a->ev) { HIP_IGNORE(hipEventSynchronize(a->ev)); HIP_IGNORE(hipEventDestroy(a->ev)); }
    if (a->words) HIP_IGNORE(hipFree(a->words));
    if (a->d_tiles) HIP_IGNORE(hipFree(a->d_tiles));
    if (a->tab_ev) { HIP_IGNORE(hipEventSynchronize(a->tab_ev)); HIP_IGNORE(hipEventDestroy(a->tab_ev)); }
    if (a->d_tab) HIP_IGNORE(hipFree(a->d_tab));
    if (a->h_tab) HIP_IGNORE(hipHostFree(a->h_tab));
    delete a;
    return 0;
}

int rtw_render_accum_f32(rtw_scene_handle scene, const rtw_camera_f32 *cam, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count,
                         rtw_accum_handle a, void *d_out, void *stream) {
    return render_accum(scene, cam, p, chunk_begin, chunk_count, a, d_out, stream);
}
int rtw_render_accum_f64(rtw_scene_handle scene, const rtw_camera_f64 *cam, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count,
                         rtw_accum_handle a, void *d_out, void *stream) {
    return render_accum(scene, cam, p, chunk_begin, chunk_count, a, d_out, stream);
}

int rtw_render_adaptive_f32(rtw_scene_handle scene, const rtw_camera_f32 *cam, const rtw_params *p, const rtw_adaptive_t *adaptive,
                            rtw_accum_handle a, void *d_out, void *stream) {
    return render_adaptive(scene, cam, p, adaptive, a, d_out, stream);
}
int rtw_render_adaptive_f64(rtw_scene_handle scene, const rtw_camera_f64 *cam, const rtw_params *p, const rtw_adaptive_t *adaptive,
                            rtw_accum_handle a, void *d_out, void *stream) {
    return render_adaptive(scene, cam, p, adaptive, a, d_out, stream);
}

int rtw_render_accum_batch_f32(rtw_scene_handle scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, int32_t chunk_begin,
                               int32_t chunk_count, const rtw_accum_handle *accums, void *d_out, void *stream) {
    return render_accum_batch(scene, cams, n_views, seeds, p, chunk_begin, chunk_count, accums, d_out, stream);
}
int rtw_render_accum_batch_f64(rtw_scene_handle scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, int32_t chunk_begin,
                               int32_t chunk_count, const rtw_accum_handle *accums, void *d_out, void *stream) {
    return render_accum_batch(scene, cams, n_views, seeds, p, chunk_begin, chunk_count, accums, d_out, stream);
}
int rtw_render_adaptive_batch_f32(rtw_scene_handle scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p,
                                  const rtw_adaptive_t *adaptive, const rtw_accum_handle *accums, void *d_out, void *stream) {
    return render_adaptive_batch(scene, cams, n_views, seeds, p, adaptive, accums, d_out, stream);
}
int rtw_render_adaptive_batch_f64(rtw_scene_handle scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p,
                                  const rtw_adaptive_t *adaptive, const rtw_accum_handle *accums, void *d_out, void *stream) {
    return render_adaptive_batch(scene, cams, n_views, seeds, p, adaptive, accums, d_out, stream);
}

int rtw_accum_adaptive_info(rtw_accum_handle a, rtw_adaptive_info_t *out) {
    if (!a || !out) return fail(-1, "null argument");
    if (!a->adaptive || a->tile_chunks.empty()) return fail(-2, "the accumulator is not adaptive");
    return adaptive_info(a, out);
}

int rtw_accum_tile_chunks(rtw_accum_handle a, int32_t capacity, int32_t *count, int32_t *chunks) {
    if (!a || !count || capacity < 0 || (capacity > 0 && !chunks)) return fail(-1, "null argument");
    const int n = n_tiles_of(a);
    if (!a->adaptive && a->ranges.size() > 1) return fail(-2, "the accumulator's chunks are not one prefix: its tiles have no chunk count");
    if (!a->adaptive && a->ranges.size() == 1 && a->ranges[0].first != 0) return fail(-2, "the accumulator's chunks are not one prefix: its tiles have no chunk count");
    *count = n;
    const int32_t uniform = a->ranges.empty() ? 0 : a->ranges[0].second;
    for (int32_t k = 0; k < capacity && k < n; ++k) chunks[k] = a->adaptive && !a->tile_chunks.empty() ? a->tile_chunks[(size_t)k] : uniform;
    return 0;
}

int rtw_accum_features_f32(rtw_scene_handle scene, const rtw_camera_f32 *cam, const rtw_params *p, rtw_accum_handle a, void *d_out, void *stream) {
    return accum_features(scene, cam, p, a, d_out, stream);
}
int rtw_accum_features_f64(rtw_scene_handle scene, const rtw_camera_f64 *cam, const rtw_params *p, rtw_accum_handle a, void *d_out, void *stream) {
    return accum_features(scene, cam, p, a, d_out, stream);
}
static int accum_noise(rtw_accum_handle a, bool f64, void *d_out, void *stream) {
    if (!a || !d_out) return fail(-1, "null argument");
    if (int rc = validate_accum_noise(a, f64)) return rc;
    if ((uintptr_t)d_out & (f64 ? 7u : 3u)) return fail(-2, "the noise map must be aligned to its element type");
    DeviceGuard guard;
    return enqueue_accum_noise(a, f64, d_out, (hipStream_t)stream);
}
int rtw_accum_noise_f32(rtw_accum_handle a, void *d_out, void *stream) { return accum_noise(a, false, d_out, stream); }
int rtw_accum_noise_f64(rtw_accum_handle a, void *d_out, void *stream) { return accum_noise(a, true, d_out, stream); }

int rtw_accum_resolve_f32(rtw_accum_handle a, int32_t gamma, void *d_out, void *stream) {
    if (!a || !d_out) return fail(-1, "null argument");
    DeviceGuard guard;
    return resolve_dev<float>(a, gamma, d_out, (hipStream_t)stream);
}
int rtw_accum_resolve_f64(rtw_accum_handle a, int32_t gamma, void *d_out, void *stream) {
    if (!a || !d_out) return fail(-1, "null argument");
    DeviceGuard guard;
    return resolve_dev<double>(a, gamma, d_out, (hipStream_t)stream);
}
int rtw_accum_resolve_batch_f32(const rtw_accum_handle *accums, int32_t n_views, int32_t gamma, void *d_out, void *stream) { return resolve_batch<float>(accums, n_views, gamma, d_out, stream); }
int rtw_accum_resolve_batch_f64(const rtw_accum_handle *accums, int32_t n_views, int32_t gamma, void *d_out, void *stream) { return resolve_batch<double>(accums, n_views, gamma, d_out, stream); }
int rtw_accum_features_batch_f32(rtw_scene_handle scene, const rtw_camera_f32 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_accum_handle *accums,
                                 void *d_out, void *stream) {
    return accum_features_batch(scene, cams, n_views, seeds, p, accums, d_out, stream);
}
int rtw_accum_features_batch_f64(rtw_scene_handle scene, const rtw_camera_f64 *cams, int32_t n_views, const uint64_t *seeds, const rtw_params *p, const rtw_accum_handle *accums,
                                 void *d_out, void *stream) {
    return accum_features_batch(scene, cams, n_views, seeds, p, accums, d_out, stream);
}
static int accum_noise_batch(const rtw_accum_handle *accums, int32_t n_views, bool f64, void *d_out, void *stream) {
    if (!d_out) return fail(-1, "null argument");
    if (int rc = validate_accum_array(accums, n_views)) return rc;
    if ((uintptr_t)d_out & (f64 ? 7u : 3u)) return fail(-2, "the noise maps must be aligned to their element type");
    if (int rc = validate_accum_noise_batch(accums, n_views, f64)) return rc;
    DeviceGuard guard;
    return enqueue_accum_noise_batch(accums, n_views, f64, d_out, (hipStream_t)stream);
}
int rtw_accum_noise_batch_f32(const rtw_accum_handle *accums, int32_t n_views, void *d_out, void *stream) { return accum_noise_batch(accums, n_views, false, d_out, stream); }
int rtw_accum_noise_batch_f64(const rtw_accum_handle *accums, int32_t n_views, void *d_out, void *stream) { return accum_noise_batch(accums, n_views, true, d_out, stream); }

int rtw_accum_resolve_host_f32(rtw_accum_handle a, int32_t gamma, float *out) { return resolve_host<float>(a, gamma, out); }
int rtw_accum_resolve_host_f64(rtw_accum_handle a, int32_t gamma, double *out) { return resolve_host<double>(a, gamma, out); }

int rtw_accum_merge(rtw_accum_handle dst, rtw_accum_handle src, void *stream_v) {
    if (!dst || !src) return fail(-1, "null argument");
    if (dst == src) return fail(-2, "an accumulator cannot be merged into itself");
    if (dst->adaptive || src->adaptive) return fail(-2, "adaptive accumulators (tiles with different chunk counts) cannot be merged");
    if (dst->width != src->width || dst->height != src->height)
        return fail(-4, "accumulators of different sizes (%d x %d, %d x %d)", dst->width, dst->height, src->width, src->height);
    if (dst->device != src->device)
        return fail(-4, "accumulators on different devices (%d, %d): export / import moves one across", dst->device, src->device);
    if (!src->bound) return 0;                  // (nothing in it)
    if (dst->bound) {
        if (!same_render(dst->bind, src->bind)) return fail(-4, "the accumulators are bound to different renders");
        for (auto &r : src->ranges)
            if (overlaps(dst->ranges, r.first, r.second)) return fail(-2, "chunk range [%d, %d) is in both accumulators", r.first, r.second);
    }
    DeviceGuard guard;
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_TRY(hipSetDevice(dst->device));
    if (int rc = wait_for(dst, stream)) return rc;
    if (int rc = wait_for(src, stream)) return rc;
    (void)hipGetLastError();
    launch_merge(stream, dst->words, src->words, n_pixels(dst));
    HIP_TRY(hipGetLastError());
    dst->bind = src->bind; dst->bound = true;
    for (auto &r : src->ranges) add_range(dst->ranges, r.first, r.second);
    if (int rc = mark(dst, stream)) return rc;
    return mark(src, stream);                   // (src is read by the merge: a later reset / pass of src waits for it)
}

int rtw_accum_info(rtw_accum_handle a, rtw_accum_info_t *out) {
    if (!a || !out) return fail(-1, "null argument");
    memset(out, 0, sizeof *out);
    out->width = a->width; out->height = a->height; out->device = a->device; out->bound = a->bound ? 1 : 0;
    if (a->bound) {
        const AccumBind &b = a->bind;
        out->precision = b.is_f64 ? 64 : 32;
        out->spp = b.spp; out->chunk_spp = b.chunk_spp; out->n_chunks = b.n_chunks; out->max_depth = b.max_depth;
        out->seed = b.seed; out->numerics_flags = b.numerics;
        out->chunks_done = chunks_done(a);
        out->samples_done = (int32_t)samples_done(a);
        out->complete = a->adaptive ? (a->ad_complete ? 1 : 0) : out->chunks_done == b.n_chunks;
    }
    return 0;
}

int rtw_accum_ranges(rtw_accum_handle a, int32_t capacity, int32_t *count, int32_t *begin_end) {
    if (!a || !count || capacity < 0 || (capacity > 0 && !begin_end)) return fail(-1, "null argument");
    *count = (int32_t)a->ranges.size();
    for (int32_t k = 0; k < capacity && k < *count; ++k) { begin_end[2 * k] = a->ranges[(size_t)k].first; begin_end[2 * k + 1] = a->ranges[(size_t)k].second; }
    return 0;
}

int rtw_accum_read_pixels(rtw_accum_handle a, uint64_t *host_words) {
    if (!a || !host_words) return fail(-1, "null argument");
    DeviceGuard guard;
    return read_words(a, host_words);
}

int rtw_accum_export(rtw_accum_handle a, void *buf, uint64_t capacity, uint64_t *size) {
    if (!a || !size) return fail(-1, "null argument");
    if (a->adaptive) return fail(-2, "adaptive accumulators (tiles with different chunk counts) cannot be exported");
    const size_t head = sizeof(BlobHeader) + a->ranges.size() * 8u, total = head + n_pixels(a) * 64u;
    *size = total;
    if (!buf) return 0;                         // (a size query)
    if (capacity < total) return fail(-2, "export needs %llu bytes, the buffer holds %llu", (unsigned long long)total, (unsigned long long)capacity);
    BlobHeader h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, "RTWACCUM", 8);
    h.version = RTW_ACCUM_BLOB_VERSION; h.header_bytes = (uint32_t)sizeof(BlobHeader);
    h.width = a->width; h.height = a->height; h.bound = a->bound ? 1 : 0; h.n_ranges = (int32_t)a->ranges.size();
    h.bind = a->bind;
    unsigned char *o = static_cast<unsigned char *>(buf);
    memcpy(o, &h, sizeof h);
    for (size_t k = 0; k < a->ranges.size(); ++k) {
        const int32_t r[2] = {a->ranges[k].first, a->ranges[k].second};
        memcpy(o + sizeof h + 8u * k, r, 8);
    }
    DeviceGuard guard;
    return read_words(a, o + head);
}

int rtw_accum_import(int device, const void *buf, uint64_t size, rtw_accum_handle *out) {
    if (!buf || !out) return fail(-1, "null argument");
    if (size < sizeof(BlobHeader)) return fail(-2, "truncated accumulator blob (%llu bytes)", (unsigned long long)size);
    BlobHeader h;
    memcpy(&h, buf, sizeof h);
    if (memcmp(h.magic, "RTWACCUM", 8) != 0) return fail(-2, "not an accumulator blob");
    if (h.version != RTW_ACCUM_BLOB_VERSION || h.header_bytes != sizeof(BlobHeader))
        return fail(-2, "accumulator blob of version %u (this library reads version %u)", h.version, RTW_ACCUM_BLOB_VERSION);
    if (int rc = check_size(h.width, h.height)) return rc;
    if (h.n_ranges < 0 || h.n_ranges > (1 << 24) || (h.bound == 0) != (h.n_ranges == 0)) return fail(-2, "corrupt accumulator blob (%d ranges)", h.n_ranges);
    const size_t head = sizeof(BlobHeader) + (size_t)h.n_ranges * 8u, total = head + (size_t)h.width * (size_t)h.height * 64u;
    if (size != total) return fail(-2, "truncated accumulator blob: %llu bytes, %llu expected", (unsigned long long)size, (unsigned long long)total);
    if (h.bound && (h.bind.spp < 1 || h.bind.chunk_spp < 1 || h.bind.n_chunks != (int32_t)(((long long)h.bind.spp + h.bind.chunk_spp - 1) / h.bind.chunk_spp)))
        return fail(-2, "corrupt accumulator blob (render)");
    const unsigned char *in = static_cast<const unsigned char *>(buf);
    std::vector<std::pair<int32_t, int32_t>> ranges;
    int32_t prev = 0;
    for (int32_t k = 0; k < h.n_ranges; ++k) {
        int32_t r[2];
        memcpy(r, in + sizeof h + 8u * (size_t)k, 8);
        if (r[0] < prev || r[1] <= r[0] || r[1] > h.bind.n_chunks) return fail(-2, "corrupt accumulator blob (range %d)", k);
        prev = r[1];
        ranges.emplace_back(r[0], r[1]);
    }
    DeviceGuard guard;
    rtw_accum_handle a = nullptr;
    // (the words are copied through an aligned staging vector: the blob's payload offset need not be a multiple of 8)
    std::vector<unsigned long long> words((size_t)h.width * (size_t)h.height * 8u);
    memcpy(words.data(), in + head, words.size() * 8u);
    if (int rc = create(device, h.width, h.height, words.data(), &a)) return rc;
    a->bound = h.bound != 0; a->bind = h.bind; a->ranges.swap(ranges);
    if (!a->bound) memset(&a->bind, 0, sizeof a->bind);
    *out = a;
    return 0;
}

}  // extern "C"
