// rtw_accum.hip -- progressive render (include/rtw_hip.h rtw_accum_*, rtw_render_accum_*): the accumulator object, the checks of a
// pass, the merge and resolve kernels, and the export / import blob.
//
// An accumulator is W x H pixels x 8 uint64 in HBM (the job slot's own layout, rtw_kernels.hpp AccumArgs) plus, on the host, the render it
// is bound to and the chunk ranges it already holds.  Every sample is a signed 64.64 integer and integer addition is associative, so ANY
// partition of a render's chunks into passes -- in any order, in any mix of scan modes and job sizes, on one accumulator or merged from
// several -- resolves to the bits of the single render.  Nothing here needs an atomic: within a launch one workgroup owns a pixel, and
// everything that touches an accumulator is ordered behind its event (`ev`: recorded after every pass / merge / reset, waited for by
// whatever comes next on whichever stream).
#include "rtw_host.hpp"
#include "rtw_path.hpp"         // fx_to_double

// what an accumulator is bound to by its first pass: everything that decides the value of a sample
struct AccumBind {
    int32_t is_f64, spp, chunk_spp, n_chunks, max_depth, numerics;
    uint64_t seed, scene_hash;
    unsigned char cam[sizeof(rtw_camera_f64)];     // the camera's bytes (Float32: the first half, the rest 0)
};

struct rtw_accum {
    int device = -1;
    int32_t width = 0, height = 0;
    unsigned long long *words = nullptr;           // device memory: width * height * 8
    hipEvent_t ev = nullptr;                       // behind the last operation enqueued on `words`
    bool bound = false;
    AccumBind bind;
    std::vector<std::pair<int32_t, int32_t>> ranges;    // chunk ranges [begin, end) already added: sorted, disjoint, coalesced
};

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

// dst += src: lane = one 16-byte pair of one pixel -- a channel's (lo, hi) (128-bit add with carry) or (poison, 0) (plain add)
__global__ __launch_bounds__(256) void accum_merge_kernel(ulonglong2 *__restrict__ dst, const ulonglong2 *__restrict__ src, size_t n_pairs) {
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n_pairs) return;
    const ulonglong2 a = dst[k], b = src[k];
    ulonglong2 r;
    r.x = a.x + b.x;
    r.y = a.y + b.y + (((k & 3u) != 3u && r.x < a.x) ? 1ull : 0ull);
    dst[k] = r;
}

// accumulator -> RGB{T} frame: store_job's formula (rtw_kernels.hpp) with the divisor `samples`; lane = (pixel, channel)
template <typename T>
__global__ __launch_bounds__(256) void accum_resolve_kernel(const unsigned long long *__restrict__ words, T *__restrict__ out, size_t n_elems, int samples, int gamma) {
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n_elems) return;
    const size_t pix = k / 3u;
    const unsigned ch = (unsigned)(k - pix * 3u);
    const unsigned long long *a = words + pix * 8u;
    double v = rtw::fx_to_double(a[2 * ch], a[2 * ch + 1]);
    if (a[6] != 0ull) v = __builtin_nan("");
    v = v / (double)samples;
    if (gamma) v = __builtin_sqrt(v);
    out[k] = (T)v;
}

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
    const size_t n = n_pixels(a) * 3u;
    (void)hipGetLastError();
    hipLaunchKernelGGL(accum_resolve_kernel<T>, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, stream, a->words, (T *)d_out, n, (int)s, (int)gamma);
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
template <typename CamT>
int validate_accum(rtw_scene_handle scene, const CamT *cam, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, rtw_accum_handle a, int *nch_out, int *cs_out) {
    if (!p) return fail(-1, "null params");
    if (!cam || !a || !scene) return fail(-1, "null argument");
    int nch, cs;
    if (int rc = validate_params(p, &nch, &cs)) return rc;
    if (p->shard_count != 1) return fail(-2, "a progressive render renders whole frames (shard_count = %d)", p->shard_count);
    if (p->flags & RTW_FLAG_COMPACT_TILES) return fail(-2, "a progressive render accumulates whole frames (RTW_FLAG_COMPACT_TILES is a per-shard layout)");
    if (p->flags & RTW_FLAG_RCCL_REDUCE) return fail(-2, "a progressive render runs on one device (RTW_FLAG_RCCL_REDUCE)");
    if (p->flags & RTW_FLAG_RAY_POOL) return fail(-2, "a progressive render runs the lane-loop kernel (RTW_FLAG_RAY_POOL)");
    if (p->n_devices > 1 || p->n_devices < 0 || p->device_ids)
        return fail(-2, "a progressive render runs on one device (n_devices = %d%s)", p->n_devices, p->device_ids ? ", device_ids given" : "");
    if (chunk_begin < 0 || chunk_count < 1 || (long long)chunk_begin + chunk_count > nch)
        return fail(-2, "chunk range [%d, %lld) is not inside the render's %d chunks", chunk_begin, (long long)chunk_begin + chunk_count, nch);
    if (scene->is_f64 != (sizeof(CamT) == sizeof(rtw_camera_f64))) return fail(-4, "scene handle precision does not match the call");
    if (a->width != p->width || a->height != p->height)
        return fail(-4, "the accumulator is %d x %d, the render %d x %d", a->width, a->height, p->width, p->height);
    if (a->device != scene->device) return fail(-4, "accumulator on device %d, scene on device %d", a->device, scene->device);
    if (p->device >= 0 && p->device != scene->device) return fail(-4, "params.device %d != scene device %d", p->device, scene->device);
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

template <typename CamT>
int render_accum(rtw_scene_handle scene, const CamT *cam, const rtw_params *p, int32_t chunk_begin, int32_t chunk_count, rtw_accum_handle a, void *d_out, void *stream_v) {
    int nch, cs;
    if (int rc = validate_accum(scene, cam, p, chunk_begin, chunk_count, a, &nch, &cs)) return rc;
    AccumBind b;
    make_bind(&b, scene, cam, p, nch, cs);
    DeviceGuard guard;
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_TRY(hipSetDevice(a->device));
    if (int rc = wait_for(a, stream)) return rc;
    AccumPass pass;
    pass.words = a->words; pass.chunk_begin = chunk_begin; pass.chunk_count = chunk_count;
    pass.samples = (int)(samples_done(a) + samples_in(b, chunk_begin, (long long)chunk_begin + chunk_count));
    RenderRec *rec = nullptr;
    CtxPtr ctx;
    release_last();
    int rc = launch_accum_t(scene, cam, p, pass, d_out, stream, &rec, &ctx);
    if (rec) { g_last.recs.push_back(rec); g_last.ctxs.push_back(ctx); }       // (also on a late error: released by the next call)
    if (rc) return rc;
    a->bind = b; a->bound = true;
    add_range(a->ranges, chunk_begin, chunk_begin + chunk_count);
    return mark(a, stream);
}

}  // namespace

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
    return mark(a, stream);
}

int rtw_accum_free(rtw_accum_handle a) {
    if (!a) return 0;
    DeviceGuard guard;
    HIP_IGNORE(hipSetDevice(a->device));
    if (a->ev) { HIP_IGNORE(hipEventSynchronize(a->ev)); HIP_IGNORE(hipEventDestroy(a->ev)); }
    if (a->words) HIP_IGNORE(hipFree(a->words));
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
int rtw_accum_resolve_host_f32(rtw_accum_handle a, int32_t gamma, float *out) { return resolve_host<float>(a, gamma, out); }
int rtw_accum_resolve_host_f64(rtw_accum_handle a, int32_t gamma, double *out) { return resolve_host<double>(a, gamma, out); }

int rtw_accum_merge(rtw_accum_handle dst, rtw_accum_handle src, void *stream_v) {
    if (!dst || !src) return fail(-1, "null argument");
    if (dst == src) return fail(-2, "an accumulator cannot be merged into itself");
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
    const size_t n = n_pixels(dst) * 4u;
    (void)hipGetLastError();
    hipLaunchKernelGGL(accum_merge_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, stream, reinterpret_cast<ulonglong2 *>(dst->words),
                       reinterpret_cast<const ulonglong2 *>(src->words), n);
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
        out->complete = out->chunks_done == b.n_chunks;
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
