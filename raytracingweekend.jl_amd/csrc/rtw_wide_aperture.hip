// rtw_wide_aperture.hip -- the wide-aperture stage (include/rtw_hip.h rtw_wide_aperture_*) and the lens family's batch: the six launches --
// the defocus stage's two kernels as rtw_defocus.hip launches them, at the full and at the reduced size, and the two kernels of
// rtw_wide_aperture.hpp --, for one view or a batch of views; the checks of N views and of a batch's frame (built from validate_lens and
// its parts in rtw_defocus.hip), the lens table, and lens_device: the ONE device-resident entry point behind rtw_defocus_device_*,
// rtw_wide_aperture_device_* and rtw_lens_batch_device_*.  Byte arithmetic: rtw_layout.hpp WideApertureLayout, LensBatchLayout.
// (The host-buffer entry points live with the other cached-context paths: lens_host in rtw_stage_host.hip, render_host_lens in
// rtw_render_host.hip.)
#include "rtw_host.hpp"
#include "rtw_wide_aperture.hpp"

namespace rtwh {

static_assert(rtw::WA_MAX_RADIUS == RTW_WIDE_APERTURE_MAX_RADIUS, "the header's bound");

// the stage's parameters as the defocus stage's (the same fields in the same order: rtw_host.hpp AsWideAperture is the way back)
static rtw_defocus_t as_defocus(const rtw_wide_aperture_t *b) {
    rtw_defocus_t d;
    memcpy(&d, b, sizeof d);
    return d;
}

// Enqueue the stage on `stream` of the current device (validate_lens has accepted the call): SIX launches, no record.
// vb null: one view.  vb given: vb->n_views views in the same six launches -- cam and d's lens are unused (the table); every region of the
// workspace lies at the single stage's offset inside its view's workspace, so one stride serves all of them.
template <typename T, int S, typename CamT>
static int launch_scaled(const rtw_defocus_t *d, const CamT *cam, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_work, void *d_out, hipStream_t stream,
                         const LensViews *vb) {
    using V = typename rtw::DnVec<T>::type;
    const WideApertureLayout L(width, height, d->max_radius);
    T *work = (T *)d_work;
    T *n_coc = work, *n_tile = work + (size_t)width * (size_t)height * 4;
    T *coc = work + L.off_coc, *tile = work + L.off_tile, *narrow = work + L.off_n;
    T *lo_img = work + L.off_lo_img, *lo_coc = work + L.off_lo_coc, *lo_tile = work + L.off_lo_tile, *lo_out = work + L.off_lo_out;
    const unsigned tiles = (unsigned)WideApertureLayout::tiles(width, height), lo_tiles = (unsigned)WideApertureLayout::tiles(L.lo_width, L.lo_height);
    const int32_t nv = vb ? vb->n_views : 0;
    const void *tab = vb ? vb->d_table : nullptr;
    const long long si = vb ? vb->img_stride : 0, sf = vb ? vb->feat_stride : 0, sw = vb ? vb->work_stride : 0, so = vb ? vb->out_stride : 0;
    const long long s_prepare[4] = {si, sf, sw, sw}, s_gather[4] = {si, sw, sw, sw}, s_small[4] = {sw, sw, sw, sw};
    // (measurement aid, tools/gpu_wide_aperture.py: events around every launch, reported on stderr -- this one blocks)
    static const bool profile = aid_flag("RTW_TEMPORAL_PROFILE");
    StageMarks marks(profile, stream);
    HIP_TRY(marks.mark());
    // 1, 2: the narrow frame N -- the defocus stage with max_radius 8, linear
    if (int rc = launch_defocus_prepare<T>(d, RTW_DEFOCUS_MAX_RADIUS, cam, width, height, d_image, d_features, n_coc, n_tile, stream, nv, tab, s_prepare)) return rc;
    HIP_TRY(marks.mark());
    if (int rc = launch_defocus_gather<T>(width, height, RTW_DEFOCUS_MAX_RADIUS, 0, d_image, n_coc, n_tile, narrow, stream, nv, s_gather)) return rc;
    HIP_TRY(marks.mark());
    // 3: the wide CoC plane
    if (int rc = launch_defocus_prepare<T>(d, d->max_radius, cam, width, height, d_image, d_features, coc, tile, stream, nv, tab, s_prepare)) return rc;
    HIP_TRY(marks.mark());
    // 4: the reduced frame
    (void)hipGetLastError();
    if (nv) hipLaunchKernelGGL((rtw::wa_reduce<T, S, true>), lens_views_grid(lo_tiles, nv), dim3(256), 0, stream, width, height, (const T *)d_image, (const V *)coc, lo_img, (V *)lo_coc, lo_tile,
                               rtw::DfViews<T, true, 5>{{si, sw, sw, sw, sw}, (unsigned)nv});
    else hipLaunchKernelGGL((rtw::wa_reduce<T, S, false>), dim3(lo_tiles), dim3(256), 0, stream, width, height, (const T *)d_image, (const V *)coc, lo_img, (V *)lo_coc, lo_tile,
                            rtw::DfViews<T, false, 5>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(marks.mark());
    // 5: the small gather
    if (int rc = launch_defocus_gather<T>(L.lo_width, L.lo_height, L.lo_mmax, 0, lo_img, lo_coc, lo_tile, lo_out, stream, nv, s_small)) return rc;
    HIP_TRY(marks.mark());
    // 6: the blend by radius
    (void)hipGetLastError();
    if (nv) hipLaunchKernelGGL((rtw::wa_compose<T, S, true>), lens_views_grid(tiles, nv), dim3(256), 0, stream, width, height, d->gamma, (const V *)coc, (const T *)narrow, (const V *)lo_coc,
                               (const T *)lo_out, (T *)d_out, rtw::DfViews<T, true, 5>{{sw, sw, sw, sw, so}, (unsigned)nv});
    else hipLaunchKernelGGL((rtw::wa_compose<T, S, false>), dim3(tiles), dim3(256), 0, stream, width, height, d->gamma, (const V *)coc, (const T *)narrow, (const V *)lo_coc, (const T *)lo_out,
                            (T *)d_out, rtw::DfViews<T, false, 5>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(marks.mark());
    if (profile) {
        const float *ms = marks.ms;
        char views[32] = "";
        if (nv) snprintf(views, sizeof views, " n_views=%d", nv);
        HIP_TRY(marks.measure());
        fprintf(stderr, "[rtw wide_aperture] %s %dx%d max_radius=%d%s prepare_ms=%.5f gather_ms=%.5f wide_prepare_ms=%.5f reduce_ms=%.5f small_gather_ms=%.5f compose_ms=%.5f\n",
                sizeof(T) == 8 ? "f64" : "f32", width, height, d->max_radius, views, ms[0], ms[1], ms[2], ms[3], ms[4], ms[5]);
    }
    return 0;
}

template <typename T, typename CamT>
int launch_wide_aperture(const rtw_wide_aperture_t *b, const CamT *cam, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_work, void *d_out, hipStream_t stream,
                                const LensViews *vb) {
    const rtw_defocus_t d = as_defocus(b);
    if (d.max_radius <= RTW_DEFOCUS_MAX_RADIUS) return launch_defocus<T>(&d, cam, width, height, d_image, d_features, d_work, d_out, stream, vb);     // (scale 1: the defocus stage itself)
    if (d.max_radius <= 16) return launch_scaled<T, 2>(&d, cam, width, height, d_image, d_features, d_work, d_out, stream, vb);
    return launch_scaled<T, 4>(&d, cam, width, height, d_image, d_features, d_work, d_out, stream, vb);
}

// ---- the batch (rtw_lens_batch_*, rtw_lens_table_*) -----------------------------------------------------------------------------
// the batch's own size rule: the batched filter's frame rule on (width, height, number of views)
static int check_views_size(int32_t width, int32_t height, int32_t n_views) {
    if ((double)width * (double)height * (double)n_views >= (double)(1ll << 39)) return fail(-5, "batch too large for one call: %d views of %d x %d pixels", n_views, width, height);
    return 0;
}

template <typename CamT>
int validate_lens_batch(const rtw_wide_aperture_t *b, const CamT *cams, int32_t n_views, int32_t width, int32_t height, const double *lens_radii, const double *focus_dists, bool own_lens, int top,
                        std::vector<rtw_defocus_t> *lens_out) {
    if (!b || !cams) return fail(-1, "null lens parameters or cameras");
    if (n_views < 1) return fail(-2, "n_views must be >= 1 (got %d)", n_views);
    if (lens_out) lens_out->clear();
    for (int32_t v = 0; v < n_views; ++v) {
        rtw_defocus_t bv = as_defocus(b);
        if (lens_radii) bv.lens_radius = lens_radii[v];
        if (focus_dists) bv.focus_dist = focus_dists[v];
        if (own_lens && bv.lens_radius == -1) bv.lens_radius = (double)cams[v].lens_radius;       // (the one-call forms alone, here and only here: the camera's own aperture)
        if (int rc = validate_lens(&bv, cams + v, width, height, top)) {
            if (n_views > 1 || lens_radii || focus_dists) {
                const std::string why = g_err;
                return fail(rc, "view %d: %s", v, why.c_str());
            }
            return rc;
        }
        if (lens_out) lens_out->push_back(bv);
    }
    return check_views_size(width, height, n_views);
}
template <typename T, typename CamT>
void lens_table(const std::vector<rtw_defocus_t> &lens, const CamT *cams, int32_t width, T *table) {
    for (size_t v = 0; v < lens.size(); ++v) lens_table_entry<T>(&lens[v], cams + v, width, table + 32 * v);
}

// What a batched entry point checks of its counts and frame before it looks at a view.  The device form stops here: it has no camera and
// reads no lens, so of validate_lens's four parts the parameters and the frame remain, with their codes.
int validate_lens_batch_frame(const rtw_wide_aperture_t *b, int32_t n_views, int32_t n_frames, int32_t width, int32_t height, int elem_bytes) {
    if (!b) return fail(-1, "null lens parameters");
    if (n_views < 1) return fail(-2, "n_views must be >= 1 (got %d)", n_views == LENS_NO_VIEWS ? 0 : n_views);     // (lens_batch_views: the caller's 0)
    if (n_frames != 1 && n_frames != n_views) return fail(-2, "n_frames must be 1 (every view reads one frame) or n_views (got %d for %d views)", n_frames, n_views);
    const rtw_defocus_t d = as_defocus(b);
    if (int rc = check_lens_params(&d, RTW_WIDE_APERTURE_MAX_RADIUS)) return rc;
    if (int rc = check_lens_frame(width, height, elem_bytes)) return rc;
    return check_views_size(width, height, n_views);
}

// The device-resident entry point of the family (rtw_defocus_device_*, rtw_wide_aperture_device_*: n_views == 0, one view of `cam` with
// max_radius in 1..top and no table; rtw_lens_batch_device_*: n_views views, their lenses in d_table, no camera): nulls, the
// parameters -- a batch's counts and frame --, then the pointers' alignment and their aliasing over the extents of the whole call (a batch's
// inputs counted once when n_frames == 1), then the launches.
template <typename T, typename CamT>
static int lens_device(int top, const rtw_wide_aperture_t *b, const CamT *cam, int32_t n_views, int32_t n_frames, const void *d_table, int32_t width, int32_t height, const void *d_image,
                       const void *d_features, void *d_work, void *d_out, void *stream_v) {
    if (!b || (n_views ? !d_table : !cam) || !d_image || !d_features || !d_work || !d_out) return fail(-1, "null argument");
    if (int rc = n_views ? validate_lens_batch_frame(b, n_views, n_frames, width, height, (int)sizeof(T)) : validate_lens_batch(b, cam, 1, width, height, nullptr, nullptr, false, top, nullptr)) return rc;
    if (((uintptr_t)d_table & 15u) || ((uintptr_t)d_features & 15u) || ((uintptr_t)d_work & 15u))
        return fail(-2, "%s must be 16-byte aligned", n_views ? "the table, the feature buffer and the workspace" : "the feature buffer and the workspace");
    if (((uintptr_t)d_image & (sizeof(T) - 1)) || ((uintptr_t)d_out & (sizeof(T) - 1))) return fail(-2, "the image buffers must be aligned to their element type");
    const LensBatchLayout R(sizeof(T), width, height, b->max_radius, n_views, n_frames);
    if (int rc = check_alias({{"d_out", d_out, R.out_b}, {"d_work", d_work, R.work_b}},
                             {{n_views ? "d_images" : "d_image", d_image, R.img_b}, {"d_features", d_features, R.feat_b}, {"d_table", d_table, R.tab_b}})) return rc;
    DeviceGuard guard;
    if (b->device >= 0) HIP_TRY(hipSetDevice(b->device));
    const LensViews vb = lens_views(R, n_views, d_table);
    return launch_wide_aperture<T>(b, cam, width, height, d_image, d_features, d_work, d_out, (hipStream_t)stream_v, n_views ? &vb : nullptr);
}

// rtw_lens_table_*: pure host code
template <typename T, typename CamT>
static int lens_table_host(const rtw_wide_aperture_t *b, const CamT *cams, int32_t n_views, int32_t width, int32_t height, const double *lens_radii, const double *focus_dists, void *table) {
    if (!b || !cams || !table) return fail(-1, "null argument");
    std::vector<rtw_defocus_t> lens;
    if (int rc = validate_lens_batch(b, cams, n_views, width, height, lens_radii, focus_dists, false, RTW_WIDE_APERTURE_MAX_RADIUS, &lens)) return rc;
    lens_table<T>(lens, cams, width, (T *)table);
    return 0;
}

template int launch_wide_aperture<float>(const rtw_wide_aperture_t *, const rtw_camera_f32 *, int32_t, int32_t, const void *, const void *, void *, void *, hipStream_t, const LensViews *);
template int launch_wide_aperture<double>(const rtw_wide_aperture_t *, const rtw_camera_f64 *, int32_t, int32_t, const void *, const void *, void *, void *, hipStream_t, const LensViews *);
template int validate_lens_batch(const rtw_wide_aperture_t *, const rtw_camera_f32 *, int32_t, int32_t, int32_t, const double *, const double *, bool, int, std::vector<rtw_defocus_t> *);
template int validate_lens_batch(const rtw_wide_aperture_t *, const rtw_camera_f64 *, int32_t, int32_t, int32_t, const double *, const double *, bool, int, std::vector<rtw_defocus_t> *);
template void lens_table<float>(const std::vector<rtw_defocus_t> &, const rtw_camera_f32 *, int32_t, float *);
template void lens_table<double>(const std::vector<rtw_defocus_t> &, const rtw_camera_f64 *, int32_t, double *);

}  // namespace rtwh

using namespace rtwh;

extern "C" {

int64_t rtw_wide_aperture_work_bytes(int32_t width, int32_t height, int32_t elem_bytes, int32_t max_radius) {
    if (const int64_t rc = rtw_denoise_work_bytes(width, height, elem_bytes); rc < 0) return rc;             // (elem_bytes, the sizes, the denoiser's frame rule)
    if (max_radius < 1 || max_radius > RTW_WIDE_APERTURE_MAX_RADIUS) return fail(-2, "max_radius must be in 1..%d (got %d)", RTW_WIDE_APERTURE_MAX_RADIUS, max_radius);
    return (int64_t)(WideApertureLayout(width, height, max_radius).total * (size_t)elem_bytes);
}
int rtw_defocus_device_f32(const rtw_defocus_t *b, const rtw_camera_f32 *cam, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_work, void *d_out,
                           void *hip_stream) {
    return lens_device<float>(RTW_DEFOCUS_MAX_RADIUS, AsWideAperture(b).ptr, cam, 0, 0, nullptr, width, height, d_image, d_features, d_work, d_out, hip_stream);
}
int rtw_defocus_device_f64(const rtw_defocus_t *b, const rtw_camera_f64 *cam, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_work, void *d_out,
                           void *hip_stream) {
    return lens_device<double>(RTW_DEFOCUS_MAX_RADIUS, AsWideAperture(b).ptr, cam, 0, 0, nullptr, width, height, d_image, d_features, d_work, d_out, hip_stream);
}
int rtw_wide_aperture_device_f32(const rtw_wide_aperture_t *b, const rtw_camera_f32 *cam, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_work,
                                 void *d_out, void *hip_stream) {
    return lens_device<float>(RTW_WIDE_APERTURE_MAX_RADIUS, b, cam, 0, 0, nullptr, width, height, d_image, d_features, d_work, d_out, hip_stream);
}
int rtw_wide_aperture_device_f64(const rtw_wide_aperture_t *b, const rtw_camera_f64 *cam, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_work,
                                 void *d_out, void *hip_stream) {
    return lens_device<double>(RTW_WIDE_APERTURE_MAX_RADIUS, b, cam, 0, 0, nullptr, width, height, d_image, d_features, d_work, d_out, hip_stream);
}

int64_t rtw_lens_table_bytes(int32_t n_views, int32_t elem_bytes) {
    if (elem_bytes != 4 && elem_bytes != 8) return fail(-2, "elem_bytes must be 4 or 8 (got %d)", elem_bytes);
    if (n_views < 1) return fail(-2, "n_views must be >= 1 (got %d)", n_views);
    return (int64_t)n_views * 32 * elem_bytes;
}
int rtw_lens_table_f32(const rtw_wide_aperture_t *b, const rtw_camera_f32 *cams, int32_t n_views, int32_t width, int32_t height, const double *lens_radii, const double *focus_dists, void *table) {
    return lens_table_host<float>(b, cams, n_views, width, height, lens_radii, focus_dists, table);
}
int rtw_lens_table_f64(const rtw_wide_aperture_t *b, const rtw_camera_f64 *cams, int32_t n_views, int32_t width, int32_t height, const double *lens_radii, const double *focus_dists, void *table) {
    return lens_table_host<double>(b, cams, n_views, width, height, lens_radii, focus_dists, table);
}
int64_t rtw_lens_batch_work_bytes(int32_t width, int32_t height, int32_t elem_bytes, int32_t max_radius, int32_t n_views) {
    const int64_t one = rtw_wide_aperture_work_bytes(width, height, elem_bytes, max_radius);
    if (one < 0) return one;
    if (n_views < 1) return fail(-2, "n_views must be >= 1 (got %d)", n_views);
    if (int rc = check_views_size(width, height, n_views)) return rc;
    return one * n_views;
}
int rtw_lens_batch_device_f32(const rtw_wide_aperture_t *b, int32_t n_views, int32_t n_frames, const void *d_table, int32_t width, int32_t height, const void *d_images,
                                       const void *d_features, void *d_work, void *d_out, void *hip_stream) {
    return lens_device<float>(RTW_WIDE_APERTURE_MAX_RADIUS, b, (const rtw_camera_f32 *)nullptr, lens_batch_views(n_views), n_frames, d_table, width, height, d_images, d_features, d_work, d_out, hip_stream);
}
int rtw_lens_batch_device_f64(const rtw_wide_aperture_t *b, int32_t n_views, int32_t n_frames, const void *d_table, int32_t width, int32_t height, const void *d_images,
                                       const void *d_features, void *d_work, void *d_out, void *hip_stream) {
    return lens_device<double>(RTW_WIDE_APERTURE_MAX_RADIUS, b, (const rtw_camera_f64 *)nullptr, lens_batch_views(n_views), n_frames, d_table, width, height, d_images, d_features, d_work, d_out, hip_stream);
}

}  // extern "C"
