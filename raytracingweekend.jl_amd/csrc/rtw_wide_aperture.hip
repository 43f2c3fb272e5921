// rtw_wide_aperture.hip -- the wide-aperture stage (include/rtw_hip.h rtw_wide_aperture_*): the checks that need no device, the workspace's
// layout (rtw_layout.hpp WideApertureLayout), the six launches -- the defocus stage's two kernels as rtw_defocus.hip launches them, at the full
// and at the reduced size, and the two kernels of rtw_wide_aperture.hpp -- and the device-resident entry points.
// (The host-buffer entry points live with the other cached-context paths: rtw_wide_aperture_* in rtw_stage_host.hip,
// rtw_render_wide_aperture_* in rtw_render_host.hip.)
#include "rtw_host.hpp"
#include "rtw_layout.hpp"
#include "rtw_wide_aperture.hpp"

namespace rtwh {

static_assert(sizeof(rtw_wide_aperture_t) == sizeof(rtw_defocus_t) && sizeof(rtw_wide_aperture_t) == 40, "the two stages' parameters have the same fields");
static_assert(rtw::WA_MAX_RADIUS == RTW_WIDE_APERTURE_MAX_RADIUS, "the header's bound");

// the stage's parameters as the defocus stage's (the same fields in the same order)
static rtw_defocus_t as_defocus(const rtw_wide_aperture_t *b) {
    rtw_defocus_t d;
    memcpy(&d, b, sizeof d);
    return d;
}

template <typename CamT>
static int validate_t(const rtw_wide_aperture_t *b, const CamT *cam, int32_t width, int32_t height) {
    if (!b || !cam) return fail(-1, "null wide-aperture parameters or camera");
    const rtw_defocus_t d = as_defocus(b);
    return validate_defocus_top(&d, cam, width, height, RTW_WIDE_APERTURE_MAX_RADIUS);
}
int validate_wide_aperture(const rtw_wide_aperture_t *b, const rtw_camera_f32 *cam, int32_t width, int32_t height) { return validate_t(b, cam, width, height); }
int validate_wide_aperture(const rtw_wide_aperture_t *b, const rtw_camera_f64 *cam, int32_t width, int32_t height) { return validate_t(b, cam, width, height); }

static int prepare_t(const rtw_defocus_t *b, int rm, const rtw_camera_f32 *c, int32_t w, int32_t h, const void *img, const void *feat, void *coc, void *tile, hipStream_t st) { return launch_defocus_prepare_f32(b, rm, c, w, h, img, feat, coc, tile, st); }
static int prepare_t(const rtw_defocus_t *b, int rm, const rtw_camera_f64 *c, int32_t w, int32_t h, const void *img, const void *feat, void *coc, void *tile, hipStream_t st) { return launch_defocus_prepare_f64(b, rm, c, w, h, img, feat, coc, tile, st); }
static int gather_t(float, int32_t w, int32_t h, int mmax, int gamma, const void *img, const void *coc, const void *tile, void *out, hipStream_t st) { return launch_defocus_gather_f32(w, h, mmax, gamma, img, coc, tile, out, st); }
static int gather_t(double, int32_t w, int32_t h, int mmax, int gamma, const void *img, const void *coc, const void *tile, void *out, hipStream_t st) { return launch_defocus_gather_f64(w, h, mmax, gamma, img, coc, tile, out, st); }

// Enqueue the stage on `stream` of the current device (validate_wide_aperture has accepted the call): SIX launches, no record.
template <typename T, int S, typename CamT>
static int launch_scaled(const rtw_defocus_t *d, const CamT *cam, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_work, void *d_out, hipStream_t stream) {
    using V = typename rtw::DnVec<T>::type;
    const WideApertureLayout L(width, height, d->max_radius);
    T *work = (T *)d_work;
    T *n_coc = work, *n_tile = work + (size_t)width * (size_t)height * 4;
    T *coc = work + L.off_coc, *tile = work + L.off_tile, *narrow = work + L.off_n;
    T *lo_img = work + L.off_lo_img, *lo_coc = work + L.off_lo_coc, *lo_tile = work + L.off_lo_tile, *lo_out = work + L.off_lo_out;
    const unsigned tiles = (unsigned)WideApertureLayout::tiles(width, height), lo_tiles = (unsigned)WideApertureLayout::tiles(L.lo_width, L.lo_height);
    // (measurement aid, tools/gpu_wide_aperture.py: events around every launch, reported on stderr -- this one blocks)
    static const bool profile = aid_flag("RTW_TEMPORAL_PROFILE");
    struct Events { hipEvent_t e[7] = {}; ~Events() { for (hipEvent_t x : e) if (x) HIP_IGNORE(hipEventDestroy(x)); } } events;
    int k = 0;
    auto mark = [&]() -> int { if (profile) HIP_TRY(hipEventRecord(events.e[k++], stream)); return 0; };
    if (profile) for (hipEvent_t &x : events.e) HIP_TRY(hipEventCreate(&x));
    if (int rc = mark()) return rc;
    // 1, 2: the narrow frame N -- the defocus stage with max_radius 8, linear
    if (int rc = prepare_t(d, RTW_DEFOCUS_MAX_RADIUS, cam, width, height, d_image, d_features, n_coc, n_tile, stream)) return rc;
    if (int rc = mark()) return rc;
    if (int rc = gather_t(T(), width, height, RTW_DEFOCUS_MAX_RADIUS, 0, d_image, n_coc, n_tile, narrow, stream)) return rc;
    if (int rc = mark()) return rc;
    // 3: the wide CoC plane
    if (int rc = prepare_t(d, d->max_radius, cam, width, height, d_image, d_features, coc, tile, stream)) return rc;
    if (int rc = mark()) return rc;
    // 4: the reduced frame
    (void)hipGetLastError();
    hipLaunchKernelGGL((rtw::wa_reduce<T, S>), dim3(lo_tiles), dim3(256), 0, stream, width, height, (const T *)d_image, (const V *)coc, lo_img, (V *)lo_coc, lo_tile);
    HIP_TRY(hipGetLastError());
    if (int rc = mark()) return rc;
    // 5: the small gather
    if (int rc = gather_t(T(), L.lo_width, L.lo_height, L.lo_mmax, 0, lo_img, lo_coc, lo_tile, lo_out, stream)) return rc;
    if (int rc = mark()) return rc;
    // 6: the blend by radius
    (void)hipGetLastError();
    hipLaunchKernelGGL((rtw::wa_compose<T, S>), dim3(tiles), dim3(256), 0, stream, width, height, d->gamma, (const V *)coc, (const T *)narrow, (const V *)lo_coc, (const T *)lo_out, (T *)d_out);
    HIP_TRY(hipGetLastError());
    if (int rc = mark()) return rc;
    if (profile) {
        float ms[6] = {0, 0, 0, 0, 0, 0};
        HIP_TRY(hipEventSynchronize(events.e[6]));
        for (int q = 0; q < 6; ++q) HIP_TRY(hipEventElapsedTime(&ms[q], events.e[q], events.e[q + 1]));
        fprintf(stderr, "[rtw wide_aperture] %s %dx%d max_radius=%d prepare_ms=%.5f gather_ms=%.5f wide_prepare_ms=%.5f reduce_ms=%.5f small_gather_ms=%.5f compose_ms=%.5f\n",
                sizeof(T) == 8 ? "f64" : "f32", width, height, d->max_radius, ms[0], ms[1], ms[2], ms[3], ms[4], ms[5]);
    }
    return 0;
}

template <typename T, typename CamT>
static int launch_wide_aperture(const rtw_wide_aperture_t *b, const CamT *cam, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_work, void *d_out, hipStream_t stream) {
    const rtw_defocus_t d = as_defocus(b);
    if (d.max_radius <= RTW_DEFOCUS_MAX_RADIUS) return launch_defocus_t(&d, cam, width, height, d_image, d_features, d_work, d_out, stream);     // (scale 1: the defocus stage itself)
    if (d.max_radius <= 16) return launch_scaled<T, 2>(&d, cam, width, height, d_image, d_features, d_work, d_out, stream);
    return launch_scaled<T, 4>(&d, cam, width, height, d_image, d_features, d_work, d_out, stream);
}

int launch_wide_aperture_f32(const rtw_wide_aperture_t *b, const rtw_camera_f32 *cam, int32_t w, int32_t h, const void *img, const void *feat, void *work, void *out, hipStream_t st) { return launch_wide_aperture<float>(b, cam, w, h, img, feat, work, out, st); }
int launch_wide_aperture_f64(const rtw_wide_aperture_t *b, const rtw_camera_f64 *cam, int32_t w, int32_t h, const void *img, const void *feat, void *work, void *out, hipStream_t st) { return launch_wide_aperture<double>(b, cam, w, h, img, feat, work, out, st); }

// The device-resident entry point: nulls, the parameters, then the pointers' alignment and aliasing.
template <typename T, typename CamT>
static int wide_aperture_device(const rtw_wide_aperture_t *b, const CamT *cam, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_work, void *d_out, void *stream_v) {
    if (!b || !cam || !d_image || !d_features || !d_work || !d_out) return fail(-1, "null argument");
    if (int rc = validate_wide_aperture(b, cam, width, height)) return rc;
    if (((uintptr_t)d_features & 15u) || ((uintptr_t)d_work & 15u)) return fail(-2, "the feature buffer and the workspace must be 16-byte aligned");
    if (((uintptr_t)d_image & (sizeof(T) - 1)) || ((uintptr_t)d_out & (sizeof(T) - 1))) return fail(-2, "the image buffers must be aligned to their element type");
    const size_t n_pix = (size_t)width * (size_t)height;
    const size_t img_b = n_pix * 3 * sizeof(T), feat_b = n_pix * 8 * sizeof(T), work_b = WideApertureLayout(width, height, b->max_radius).total * sizeof(T);
    if (int rc = check_alias({{"d_out", d_out, img_b}, {"d_work", d_work, work_b}}, {{"d_image", d_image, img_b}, {"d_features", d_features, feat_b}})) return rc;
    DeviceGuard guard;
    if (b->device >= 0) HIP_TRY(hipSetDevice(b->device));
    return launch_wide_aperture<T>(b, cam, width, height, d_image, d_features, d_work, d_out, (hipStream_t)stream_v);
}

}  // namespace rtwh

using namespace rtwh;

extern "C" {

int64_t rtw_wide_aperture_work_bytes(int32_t width, int32_t height, int32_t elem_bytes, int32_t max_radius) {
    if (const int64_t rc = rtw_denoise_work_bytes(width, height, elem_bytes); rc < 0) return rc;             // (elem_bytes, the sizes, the denoiser's frame rule)
    if (max_radius < 1 || max_radius > RTW_WIDE_APERTURE_MAX_RADIUS) return fail(-2, "max_radius must be in 1..%d (got %d)", RTW_WIDE_APERTURE_MAX_RADIUS, max_radius);
    return (int64_t)(WideApertureLayout(width, height, max_radius).total * (size_t)elem_bytes);
}
int rtw_wide_aperture_device_f32(const rtw_wide_aperture_t *b, const rtw_camera_f32 *cam, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_work,
                                 void *d_out, void *hip_stream) {
    return wide_aperture_device<float>(b, cam, width, height, d_image, d_features, d_work, d_out, hip_stream);
}
int rtw_wide_aperture_device_f64(const rtw_wide_aperture_t *b, const rtw_camera_f64 *cam, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_work,
                                 void *d_out, void *hip_stream) {
    return wide_aperture_device<double>(b, cam, width, height, d_image, d_features, d_work, d_out, hip_stream);
}

}  // extern "C"
