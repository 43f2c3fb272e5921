// rtw_defocus.hip -- the defocus stage (include/rtw_hip.h rtw_defocus_*) and what the whole lens family takes from it: the checks of one
// view that need no device, in their four parts (validate_lens), the host constants (one view's entry of the lens table) and the two
// launches of its kernels (rtw_defocus.hpp).  The workspace's size comes from rtw_layout.hpp WideApertureLayout.
// (The entry points of the family share one body per tier: lens_device in rtw_wide_aperture.hip behind rtw_defocus_device_*, lens_host in
// rtw_stage_host.hip behind rtw_defocus_*, render_host_lens in rtw_render_host.hip behind rtw_render_defocused_*.)
#include "rtw_host.hpp"
#include "rtw_defocus.hpp"

namespace rtwh {

// the host constants of the definition in binary64, every operation rounded once: the focus distance in use and the circle-of-confusion radius,
// in pixels, of a point at infinity
template <typename CamT>
static void defocus_constants(const rtw_defocus_t *b, const CamT *cam, int32_t width, double *hh, double *focus, double *K) {
    double q[3], w[3], h[3];
    for (int k = 0; k < 3; ++k) { q[k] = (double)cam->origin[k] - (double)cam->lower_left_corner[k]; w[k] = cam->w[k]; h[k] = cam->horizontal[k]; }
    *hh = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2];
    *focus = b->focus_dist > 0 ? b->focus_dist : (q[0] * w[0] + q[1] * w[1]) + q[2] * w[2];
    *K = (b->lens_radius * (double)width) / std::sqrt(*hh);
}

// One view's entry of the lens table (include/rtw_hip.h rtw_lens_table_*: 32 elements): [0, 29) the reprojection table's entry of the camera
// as its own previous one (so that element 15.. is its w), 29: F = T(focus), 30: K rounded to T, 31: 0.  The ONE copy of this arithmetic:
// launch_defocus_prepare's own constants and rtw_lens_table_* both come from here.
template <typename T, typename CamT>
void lens_table_entry(const rtw_defocus_t *b, const CamT *cam, int32_t width, T *e) {
    double hh, focus, K;
    defocus_constants(b, cam, width, &hh, &focus, &K);
    temporal_table<T>(cam, cam, 1, e);
    e[29] = (T)focus; e[30] = (T)K; e[31] = T(0);
}

// Everything about a lens stage that is decided without a device and without a pointer, in four parts, in the order every entry point of
// the family applies them.  1: the parameters -- max_radius against the stage's `top` (8: the defocus stage, 32: the wide-aperture stage and
// the batch), flags, gamma, device, reserved.
int check_lens_params(const rtw_defocus_t *b, int top) {
    if (b->max_radius < 1 || b->max_radius > top) return fail(-2, "max_radius must be in 1..%d (got %d)", top, b->max_radius);
    if (b->flags != 0) return fail(-2, "unknown defocus flags 0x%x", b->flags);
    if (b->gamma != 0 && b->gamma != 1) return fail(-2, "gamma must be 0 or 1 (got %d)", b->gamma);
    if (b->device < -1) return fail(-2, "bad device %d", b->device);
    if (b->reserved[0] != 0 || b->reserved[1] != 0) return fail(-2, "reserved must be 0");
    return 0;
}
// 2: the lens
static int check_lens_values(const rtw_defocus_t *b) {
    if (!(b->lens_radius >= 0) || !std::isfinite(b->lens_radius)) return fail(-2, "lens_radius must be finite and >= 0");
    if (!(b->focus_dist >= 0) || !std::isfinite(b->focus_dist)) return fail(-2, "focus_dist must be finite and >= 0 (0: the camera's own focus plane)");
    return 0;
}
// 3: the frame -- the sizes, then elem_bytes and the denoiser's frame rule
int check_lens_frame(int32_t width, int32_t height, int elem_bytes) {
    if (width < 1 || height < 1) return fail(-2, "width/height must be positive (got %d x %d)", width, height);
    if (const int64_t rc = rtw_denoise_work_bytes(width, height, elem_bytes); rc < 0) return (int)rc;
    return 0;
}
// 4: the camera
template <typename CamT>
static int check_lens_camera(const rtw_defocus_t *b, const CamT *cam, int32_t width) {
    double hh, focus, K;
    defocus_constants(b, cam, width, &hh, &focus, &K);
    if (!(hh > 0) || !std::isfinite(hh)) return fail(-2, "the camera's horizontal vector must have a finite, positive length");
    if (!(focus > 0) || !std::isfinite(focus)) return fail(-2, "the camera's focus distance (origin - lower_left_corner).w must be finite and positive");
    return 0;
}
template <typename CamT>
int validate_lens(const rtw_defocus_t *b, const CamT *cam, int32_t width, int32_t height, int top) {
    if (!b || !cam) return fail(-1, "null lens parameters or camera");
    if (int rc = check_lens_params(b, top)) return rc;
    if (int rc = check_lens_values(b)) return rc;
    if (int rc = check_lens_frame(width, height, (int)sizeof(cam->origin[0]))) return rc;
    return check_lens_camera(b, cam, width);
}

static_assert(rtw::DF_TILE == 16, "rtw_layout.hpp WideApertureLayout::tiles counts the kernels' 16 x 16 tiles");

// the view dimensions of a batched launch's grid: the view index is blockIdx.z * gridDim.y + blockIdx.y (rtw_defocus.hpp DfViews)
dim3 lens_views_grid(unsigned tiles, int32_t n_views) {
    const unsigned nv = (unsigned)n_views;
    return dim3(tiles, nv < rtw::DF_VIEWS_Y ? nv : rtw::DF_VIEWS_Y, (nv + rtw::DF_VIEWS_Y - 1) / rtw::DF_VIEWS_Y);
}

// The stage's two launches one by one (launch_defocus below; rtw_wide_aperture.hip composes them): launch_defocus_prepare, the prepare launch with the clamp `rm`
// over the image and the features into a CoC plane and its tile plane ...
// n_views == 0: ONE view, the constants from b and cam.  n_views >= 1 (rtw_lens_batch_device_*): that many views in the SAME single
// launch -- b and cam are unused, view v takes its constants from entry v of the DEVICE table d_table (lens_table) and finds its image,
// features, CoC plane and tile plane v * strides[0..3] bytes behind the pointers.
template <typename T, typename CamT>
int launch_defocus_prepare(const rtw_defocus_t *b, int rm, const CamT *cam, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_coc, void *d_tile, hipStream_t stream,
                           int32_t n_views, const void *d_table, const long long *strides) {
    using V = typename rtw::DnVec<T>::type;
    const unsigned tiles = (unsigned)WideApertureLayout::tiles(width, height);                 // (fewer than the frame rule's 8 x 8 ones: one 32-bit grid dimension holds them)
    rtw::TpParams<T> U;
    memset(&U, 0, sizeof U);
    T FK[2] = {T(0), T(0)};
    if (!n_views) {
        T e[32];
        lens_table_entry<T>(b, cam, width, e);
        memcpy(&U, e, 29 * sizeof(T));
        FK[0] = e[29]; FK[1] = e[30];
    }
    U.W = width; U.H = height;
    (void)hipGetLastError();
    if (n_views) {
        rtw::DfLens<T, true> B;
        for (int k = 0; k < 4; ++k) B.stride[k] = strides[k];
        B.n_views = (unsigned)n_views; B.table = (const T *)d_table;
        hipLaunchKernelGGL((rtw::df_prepare<T, true>), lens_views_grid(tiles, n_views), dim3(256), 0, stream, U, FK[0], FK[1], (T)rm, (const T *)d_image, (const V *)d_features, (V *)d_coc,
                           (T *)d_tile, B);
    } else {
        hipLaunchKernelGGL((rtw::df_prepare<T, false>), dim3(tiles), dim3(256), 0, stream, U, FK[0], FK[1], (T)rm, (const T *)d_image, (const V *)d_features, (V *)d_coc, (T *)d_tile,
                           rtw::DfLens<T, false>());
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
// ... and launch_defocus_gather, the gather of a frame of any size over its image, CoC plane and tile plane; mmax >= every radius of the plane, at most 8.
// n_views >= 1: that many frames in the same single launch, image, CoC plane, tile plane and output of view v at v * strides[0..3] bytes.
template <typename T>
int launch_defocus_gather(int32_t width, int32_t height, int mmax, int gamma, const void *d_image, const void *d_coc, const void *d_tile, void *d_out, hipStream_t stream, int32_t n_views,
                          const long long *strides) {
    using V = typename rtw::DnVec<T>::type;
    const unsigned tiles = (unsigned)WideApertureLayout::tiles(width, height);
    rtw::DfDist<T> tab;
    for (int dj = 0; dj <= rtw::DF_MAX_RADIUS; ++dj)
        for (int di = 0; di <= rtw::DF_MAX_RADIUS; ++di) tab.d[dj * (rtw::DF_MAX_RADIUS + 1) + di] = std::sqrt((T)(di * di + dj * dj));
    const size_t lds = (size_t)(rtw::DF_TILE + 2 * mmax) * rtw::DF_COL * sizeof(T);      // (at most 32 columns: 24 / 48 KB)
    (void)hipGetLastError();
    if (n_views) {
        rtw::DfViews<T, true, 4> B;
        for (int k = 0; k < 4; ++k) B.stride[k] = strides[k];
        B.n_views = (unsigned)n_views;
        hipLaunchKernelGGL((rtw::df_gather<T, true>), lens_views_grid(tiles, n_views), dim3(256), lds, stream, width, height, mmax, gamma, tab, (const T *)d_image, (const V *)d_coc,
                           (const T *)d_tile, (T *)d_out, B);
    } else {
        hipLaunchKernelGGL((rtw::df_gather<T, false>), dim3(tiles), dim3(256), lds, stream, width, height, mmax, gamma, tab, (const T *)d_image, (const V *)d_coc, (const T *)d_tile, (T *)d_out,
                           rtw::DfViews<T, false, 4>());
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// Enqueue the stage on `stream` of the current device (validate_lens has accepted the call): TWO launches, no record.
// vb null: one view.  vb given (rtw_lens_batch_device_* with max_radius <= 8): vb->n_views views in the same two launches -- cam and
// b's lens are unused (the table), the buffers hold the views at vb's strides.
template <typename T, typename CamT>
int launch_defocus(const rtw_defocus_t *b, const CamT *cam, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_work, void *d_out, hipStream_t stream,
                   const LensViews *vb) {
    using V = typename rtw::DnVec<T>::type;
    V *coc = (V *)d_work;
    T *tile = (T *)(coc + (size_t)width * (size_t)height);
    const int32_t nv = vb ? vb->n_views : 0;
    const long long sp[4] = {vb ? vb->img_stride : 0, vb ? vb->feat_stride : 0, vb ? vb->work_stride : 0, vb ? vb->work_stride : 0};
    const long long sg[4] = {sp[0], sp[2], sp[2], vb ? vb->out_stride : 0};
    // (measurement aid, tools/gpu_defocus.py: events around every launch, reported on stderr -- this one blocks)
    static const bool profile = aid_flag("RTW_TEMPORAL_PROFILE");
    StageMarks marks(profile, stream);
    HIP_TRY(marks.mark());
    if (int rc = launch_defocus_prepare<T>(b, b->max_radius, cam, width, height, d_image, d_features, coc, tile, stream, nv, vb ? vb->d_table : nullptr, sp)) return rc;
    HIP_TRY(marks.mark());
    if (int rc = launch_defocus_gather<T>(width, height, b->max_radius, b->gamma, d_image, coc, tile, d_out, stream, nv, sg)) return rc;
    if (profile) {
        const float *ms = marks.ms;
        char views[32] = "";
        if (nv) snprintf(views, sizeof views, " n_views=%d", nv);
        HIP_TRY(marks.mark());
        HIP_TRY(marks.measure());
        fprintf(stderr, "[rtw defocus] %s %dx%d max_radius=%d%s prepare_ms=%.5f gather_ms=%.5f\n", sizeof(T) == 8 ? "f64" : "f32", width, height, b->max_radius, views, ms[0], ms[1]);
    }
    return 0;
}

template void lens_table_entry<float>(const rtw_defocus_t *, const rtw_camera_f32 *, int32_t, float *);
template void lens_table_entry<double>(const rtw_defocus_t *, const rtw_camera_f64 *, int32_t, double *);
template int validate_lens(const rtw_defocus_t *, const rtw_camera_f32 *, int32_t, int32_t, int);
template int validate_lens(const rtw_defocus_t *, const rtw_camera_f64 *, int32_t, int32_t, int);
template int launch_defocus_prepare<float>(const rtw_defocus_t *, int, const rtw_camera_f32 *, int32_t, int32_t, const void *, const void *, void *, void *, hipStream_t, int32_t, const void *, const long long *);
template int launch_defocus_prepare<double>(const rtw_defocus_t *, int, const rtw_camera_f64 *, int32_t, int32_t, const void *, const void *, void *, void *, hipStream_t, int32_t, const void *, const long long *);
template int launch_defocus_gather<float>(int32_t, int32_t, int, int, const void *, const void *, const void *, void *, hipStream_t, int32_t, const long long *);
template int launch_defocus_gather<double>(int32_t, int32_t, int, int, const void *, const void *, const void *, void *, hipStream_t, int32_t, const long long *);
template int launch_defocus<float>(const rtw_defocus_t *, const rtw_camera_f32 *, int32_t, int32_t, const void *, const void *, void *, void *, hipStream_t, const LensViews *);
template int launch_defocus<double>(const rtw_defocus_t *, const rtw_camera_f64 *, int32_t, int32_t, const void *, const void *, void *, void *, hipStream_t, const LensViews *);

}  // namespace rtwh

using namespace rtwh;

extern "C" {

int64_t rtw_defocus_work_bytes(int32_t width, int32_t height, int32_t elem_bytes) {
    if (const int64_t rc = rtw_denoise_work_bytes(width, height, elem_bytes); rc < 0) return rc;             // (elem_bytes, the sizes, the denoiser's frame rule)
    return (int64_t)(WideApertureLayout(width, height, RTW_DEFOCUS_MAX_RADIUS).narrow * (size_t)elem_bytes);
}

}  // extern "C"
