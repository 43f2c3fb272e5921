// rtw_temporal.hip -- temporal reprojection (include/rtw_hip.h rtw_temporal_*): the checks that need no device, the host constants of a step,
// the one launch of its kernel (rtw_temporal.hpp), the step with moments and the noise map (rtw_history_moments_*, rtw_history_noise_device_*), the
// clamped step (rtw_clamped_step_device_*: the checks of its clamp and the launch of its own kernel, rtw_temporal_clamp.hpp) and the
// device-resident entry points.
// (The host-buffer entry points, rtw_temporal_*, rtw_history_moments_*, rtw_clamped_step_*, rtw_render_sequence_* and rtw_render_path_*, live with the other
// cached-context paths in rtw_render_host.hip.)
#include "rtw_host.hpp"
#include "rtw_temporal.hpp"
#include "rtw_temporal_clamp.hpp"

namespace rtwh {

// Everything about a temporal step that is decided without a device and without a pointer.
int validate_temporal(const rtw_temporal_t *t, int32_t width, int32_t height, int elem_bytes) {
    if (!t) return fail(-1, "null temporal parameters");
    if (t->normal_power_log2 < 0 || t->normal_power_log2 > 7) return fail(-2, "normal_power_log2 must be in 0..7 (got %d)", t->normal_power_log2);
    if (t->flags & ~(RTW_TEMPORAL_DEMODULATE)) return fail(-2, "unknown temporal flags 0x%x", t->flags);
    if (t->gamma != 0 && t->gamma != 1) return fail(-2, "gamma must be 0 or 1 (got %d)", t->gamma);
    if (t->device < -1) return fail(-2, "bad device %d", t->device);
    if (t->reserved[0] != 0 || t->reserved[1] != 0) return fail(-2, "reserved must be 0");
    if (!(t->sigma_depth > 0) || !std::isfinite(t->sigma_depth)) return fail(-2, "sigma_depth must be finite and positive");
    if (!(t->min_weight > 0) || !(t->min_weight <= 1)) return fail(-2, "min_weight must be in (0, 1]");
    if (!(t->history_max >= 1) || !std::isfinite(t->history_max)) return fail(-2, "history_max must be finite and >= 1");
    if (width < 1 || height < 1) return fail(-2, "width/height must be positive (got %d x %d)", width, height);
    if (const int64_t rc = rtw_denoise_work_bytes(width, height, elem_bytes); rc < 0) return (int)rc;         // (the denoiser's frame rule)
    return 0;
}

// Everything about the clamp of a clamped step (rtw_clamped_step_*, rtw_render_path_clamped_*) that is decided without a device and without a pointer.
int validate_temporal_clamp(const rtw_temporal_clamp_t *c) {
    if (!c) return fail(-1, "null temporal clamp parameters");
    if (c->radius < 1 || c->radius > 3) return fail(-2, "clamp radius must be in 1..3 (got %d)", c->radius);
    if (c->flags & ~(RTW_CLAMP_GUIDES)) return fail(-2, "unknown clamp flags 0x%x", c->flags);
    if (c->reserved[0] != 0 || c->reserved[1] != 0) return fail(-2, "clamp reserved must be 0");
    if (!(c->sigma >= 0) || !std::isfinite(c->sigma)) return fail(-2, "clamp sigma must be finite and >= 0");
    if (!(c->len_scale >= 0) || !(c->len_scale <= 1)) return fail(-2, "clamp len_scale must be in [0, 1]");
    return 0;
}

// the state: the planes E and G of 4 elements per pixel and L of one, one behind the other (each starts on a 16-byte boundary)
static long long state_bytes(int32_t width, int32_t height, int elem_bytes) { return ((long long)width * height * 9 * elem_bytes + 15) & ~15ll; }

// the moment plane: one element per pixel (it starts on a 16-byte boundary like a state)
static long long moment_bytes(int32_t width, int32_t height, int elem_bytes) { return ((long long)width * height * elem_bytes + 15) & ~15ll; }

// Everything about a noise map (rtw_history_noise_device_*) that is decided without a device and without a pointer.
int validate_temporal_noise(const rtw_temporal_noise_t *n, int32_t width, int32_t height, int elem_bytes) {
    if (!n) return fail(-1, "null temporal noise parameters");
    if (n->radius < 1 || n->radius > 3) return fail(-2, "radius must be in 1..3 (got %d)", n->radius);
    if (n->normal_power_log2 < 0 || n->normal_power_log2 > 7) return fail(-2, "normal_power_log2 must be in 0..7 (got %d)", n->normal_power_log2);
    if (n->device < -1) return fail(-2, "bad device %d", n->device);
    if (n->reserved[0] != 0 || n->reserved[1] != 0 || n->reserved[2] != 0) return fail(-2, "reserved must be 0");
    if (!(n->sigma_depth > 0) || !std::isfinite(n->sigma_depth)) return fail(-2, "sigma_depth must be finite and positive");
    if (!(n->min_len >= 1) || !std::isfinite(n->min_len)) return fail(-2, "min_len must be finite and >= 1");
    if (width < 1 || height < 1) return fail(-2, "width/height must be positive (got %d x %d)", width, height);
    if (const int64_t rc = rtw_denoise_work_bytes(width, height, elem_bytes); rc < 0) return (int)rc;         // (the denoiser's frame rule)
    return 0;
}

// Enqueue one step on `stream` of the current device (validate_temporal has accepted the call).  cam_prev and d_state_prev are both null
// (the first frame) or both given.  d_moment_next non-null: the step with moments (rtw_history_moments_*), d_moment_prev null exactly when
// d_state_prev is.  `c` non-null (validate_temporal_clamp has accepted it): the clamped step -- its own kernel (rtw_temporal_clamp.hpp), one workgroup per
// tile, whenever there is a previous state; the first frame is the plain step's.
template <typename T, typename CamT>
int launch_temporal(const rtw_temporal_t *t, const CamT *cam, const CamT *cam_prev, int32_t width, int32_t height, const void *d_image, const void *d_features,
                    const void *d_state_prev, void *d_state_next, void *d_out, hipStream_t stream, const void *d_moment_prev, void *d_moment_next, const rtw_temporal_clamp_t *c) {
    using V = typename rtw::DnVec<T>::type;
    const long long n_pix = (long long)width * height;
    rtw::TpParams<T> U;
    memset(&U, 0, sizeof U);
    for (int k = 0; k < 3; ++k) { U.o[k] = cam->origin[k]; U.llc[k] = cam->lower_left_corner[k]; U.hor[k] = cam->horizontal[k]; U.ver[k] = cam->vertical[k]; }
    if (cam_prev) {
        // the projection's constants: binary64 from the previous camera's fields, every dot product (x + y) + z, each rounded to T once
        double q[3], w[3], h[3], v[3];
        for (int k = 0; k < 3; ++k) {
            U.po[k] = cam_prev->origin[k]; U.pw[k] = cam_prev->w[k]; U.ph[k] = cam_prev->horizontal[k]; U.pv[k] = cam_prev->vertical[k];
            q[k] = (double)cam_prev->lower_left_corner[k] - (double)cam_prev->origin[k];
            w[k] = cam_prev->w[k]; h[k] = cam_prev->horizontal[k]; v[k] = cam_prev->vertical[k];
        }
        auto dot = [](const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; };
        U.Kw = (T)dot(q, w); U.Qh = (T)dot(q, h); U.Qv = (T)dot(q, v);
        U.ih = (T)(1.0 / dot(h, h)); U.iv = (T)(1.0 / dot(v, v));
    }
    U.inv_sz = (T)(1.0 / (t->sigma_depth * t->sigma_depth));
    U.w_min = (T)t->min_weight; U.n_max = (T)t->history_max;
    U.m = t->normal_power_log2;
    U.mode = ((t->flags & RTW_TEMPORAL_DEMODULATE) ? RTW_DN_DEMOD : 0) | (t->gamma ? RTW_DN_GAMMA : 0);
    U.W = width; U.H = height;
    const long long pb = n_pix * 4 * (long long)sizeof(T);
    const char *sp = (const char *)d_state_prev;
    char *sn = (char *)d_state_next;
    const unsigned grid = (unsigned)((n_pix + 255) / 256);
    // (measurement aid, tools/gpu_temporal.py: events around the kernel, reported on stderr -- this one blocks)
    static const bool profile = aid_flag("RTW_TEMPORAL_PROFILE");
    struct Events { hipEvent_t e[2] = {}; ~Events() { for (hipEvent_t x : e) if (x) HIP_IGNORE(hipEventDestroy(x)); } } events;
    if (profile) { for (hipEvent_t &x : events.e) HIP_TRY(hipEventCreate(&x)); HIP_TRY(hipEventRecord(events.e[0], stream)); }
    (void)hipGetLastError();
    const T *mp = (const T *)d_moment_prev;
    T *mn = (T *)d_moment_next;
    if (c && sp) {
        // the tile grid: fewer tiles than the frame rule's 8 x 8 ones, so one 32-bit grid dimension holds them
        rtw::TpClampParams<T> K;
        memset(&K, 0, sizeof K);
        K.ks = (T)c->sigma; K.ls = (T)c->len_scale; K.r = c->radius;
        K.tiles_i = (unsigned)((height + rtw::TP_TI - 1) / rtw::TP_TI);
        const unsigned tiles = K.tiles_i * (unsigned)((width + rtw::TP_TJ - 1) / rtw::TP_TJ);
        const bool gd = (c->flags & RTW_CLAMP_GUIDES) != 0;
#define RTW_TP_CLAMPED(MO, GD) hipLaunchKernelGGL((rtw::tp_step_clamped<T, MO, GD>), dim3(tiles), dim3(256), 0, stream, U, K, (const T *)d_image, (const V *)d_features, (const V *)sp, \
                                                  (const V *)(sp + pb), (const T *)(sp + 2 * pb), (V *)sn, (V *)(sn + pb), (T *)(sn + 2 * pb), (T *)d_out, mp, mn)
        if (mn) { if (gd) RTW_TP_CLAMPED(true, true); else RTW_TP_CLAMPED(true, false); }
        else { if (gd) RTW_TP_CLAMPED(false, true); else RTW_TP_CLAMPED(false, false); }
#undef RTW_TP_CLAMPED
    } else if (mn) {
        if (sp) hipLaunchKernelGGL((rtw::tp_step<T, true, true>), dim3(grid), dim3(256), 0, stream, U, (const T *)d_image, (const V *)d_features, (const V *)sp, (const V *)(sp + pb),
                                   (const T *)(sp + 2 * pb), (V *)sn, (V *)(sn + pb), (T *)(sn + 2 * pb), (T *)d_out, mp, mn);
        else hipLaunchKernelGGL((rtw::tp_step<T, false, true>), dim3(grid), dim3(256), 0, stream, U, (const T *)d_image, (const V *)d_features, (const V *)nullptr, (const V *)nullptr,
                                (const T *)nullptr, (V *)sn, (V *)(sn + pb), (T *)(sn + 2 * pb), (T *)d_out, (const T *)nullptr, mn);
    } else if (sp) hipLaunchKernelGGL((rtw::tp_step<T, true>), dim3(grid), dim3(256), 0, stream, U, (const T *)d_image, (const V *)d_features, (const V *)sp, (const V *)(sp + pb),
                                      (const T *)(sp + 2 * pb), (V *)sn, (V *)(sn + pb), (T *)(sn + 2 * pb), (T *)d_out, (const T *)nullptr, (T *)nullptr);
    else hipLaunchKernelGGL((rtw::tp_step<T, false>), dim3(grid), dim3(256), 0, stream, U, (const T *)d_image, (const V *)d_features, (const V *)nullptr, (const V *)nullptr,
                            (const T *)nullptr, (V *)sn, (V *)(sn + pb), (T *)(sn + 2 * pb), (T *)d_out, (const T *)nullptr, (T *)nullptr);
    HIP_TRY(hipGetLastError());
    if (profile) {
        float ms = 0;
        HIP_TRY(hipEventRecord(events.e[1], stream));
        HIP_TRY(hipEventSynchronize(events.e[1]));
        HIP_TRY(hipEventElapsedTime(&ms, events.e[0], events.e[1]));
        if (c && sp) fprintf(stderr, "[rtw temporal] %s %dx%d %s r=%d guides=%d ms=%.5f\n", sizeof(T) == 8 ? "f64" : "f32", width, height, mn ? "clamped+moments" : "clamped", c->radius, c->flags & RTW_CLAMP_GUIDES, ms);
        else fprintf(stderr, "[rtw temporal] %s %dx%d %s prev=%d ms=%.5f\n", sizeof(T) == 8 ? "f64" : "f32", width, height, mn ? "step+moments" : "step", sp ? 1 : 0, ms);
    }
    return 0;
}

int launch_temporal_f32(const rtw_temporal_t *t, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t w, int32_t h, const void *img, const void *feat, const void *sp, void *sn, void *out, hipStream_t st, const void *mp, void *mn, const rtw_temporal_clamp_t *c) { return launch_temporal<float>(t, cam, cam_prev, w, h, img, feat, sp, sn, out, st, mp, mn, c); }
int launch_temporal_f64(const rtw_temporal_t *t, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t w, int32_t h, const void *img, const void *feat, const void *sp, void *sn, void *out, hipStream_t st, const void *mp, void *mn, const rtw_temporal_clamp_t *c) { return launch_temporal<double>(t, cam, cam_prev, w, h, img, feat, sp, sn, out, st, mp, mn, c); }

// Enqueue the noise map of a state and its moment plane on `stream` of the current device (validate_temporal_noise has accepted the call): ONE launch.
template <typename T>
int launch_temporal_noise(const rtw_temporal_noise_t *n, int32_t width, int32_t height, const void *d_state, const void *d_moment, void *d_noise, hipStream_t stream) {
    using V = typename rtw::DnVec<T>::type;
    const long long n_pix = (long long)width * height;
    rtw::TpNoiseParams<T> U;
    memset(&U, 0, sizeof U);
    U.inv_sz = (T)(1.0 / (n->sigma_depth * n->sigma_depth));
    U.min_len = (T)n->min_len;
    U.m = n->normal_power_log2; U.r = n->radius;
    U.W = width; U.H = height;
    const long long pb = n_pix * 4 * (long long)sizeof(T);
    const char *sp = (const char *)d_state;
    const unsigned grid = (unsigned)((n_pix + 255) / 256);
    // (measurement aid, tools/gpu_temporal_noise.py: events around the kernel, reported on stderr -- this one blocks)
    static const bool profile = aid_flag("RTW_TEMPORAL_PROFILE");
    struct Events { hipEvent_t e[2] = {}; ~Events() { for (hipEvent_t x : e) if (x) HIP_IGNORE(hipEventDestroy(x)); } } events;
    if (profile) { for (hipEvent_t &x : events.e) HIP_TRY(hipEventCreate(&x)); HIP_TRY(hipEventRecord(events.e[0], stream)); }
    (void)hipGetLastError();
    hipLaunchKernelGGL((rtw::tp_noise<T>), dim3(grid), dim3(256), 0, stream, U, (const V *)sp, (const V *)(sp + pb), (const T *)(sp + 2 * pb), (const T *)d_moment, (T *)d_noise);
    HIP_TRY(hipGetLastError());
    if (profile) {
        float ms = 0;
        HIP_TRY(hipEventRecord(events.e[1], stream));
        HIP_TRY(hipEventSynchronize(events.e[1]));
        HIP_TRY(hipEventElapsedTime(&ms, events.e[0], events.e[1]));
        fprintf(stderr, "[rtw temporal] %s %dx%d noise r=%d ms=%.5f\n", sizeof(T) == 8 ? "f64" : "f32", width, height, n->radius, ms);
    }
    return 0;
}

int launch_temporal_noise_f32(const rtw_temporal_noise_t *n, int32_t w, int32_t h, const void *st, const void *mo, void *noise, hipStream_t s) { return launch_temporal_noise<float>(n, w, h, st, mo, noise, s); }
int launch_temporal_noise_f64(const rtw_temporal_noise_t *n, int32_t w, int32_t h, const void *st, const void *mo, void *noise, hipStream_t s) { return launch_temporal_noise<double>(n, w, h, st, mo, noise, s); }

// The device-resident entry points of a step: nulls, the parameters, then the pointers' alignment and aliasing.  `moments`:
// rtw_history_moments_device_*, the same with the two moment planes (d_moment_prev null exactly when d_state_prev is).  `clamped`:
// rtw_clamped_step_device_*, either of the two with the clamp `c`.
template <typename T, typename CamT>
int temporal_device(const rtw_temporal_t *t, const CamT *cam, const CamT *cam_prev, int32_t width, int32_t height, const void *d_image, const void *d_features, const void *d_state_prev,
                    void *d_state_next, void *d_out, void *stream_v, bool moments = false, const void *d_moment_prev = nullptr, void *d_moment_next = nullptr, bool clamped = false,
                    const rtw_temporal_clamp_t *c = nullptr) {
    if (!t || !cam || !d_image || !d_features || !d_state_next || !d_out || (moments && !d_moment_next) || (clamped && !c)) return fail(-1, "null argument");
    if (int rc = validate_temporal(t, width, height, (int)sizeof(T))) return rc;
    if (clamped) if (int rc = validate_temporal_clamp(c)) return rc;
    if ((cam_prev == nullptr) != (d_state_prev == nullptr)) return fail(-2, "cam_prev and d_state_prev must both be given or both be null (the first frame)");
    if (moments && (d_moment_prev == nullptr) != (d_state_prev == nullptr)) return fail(-2, "d_moment_prev and d_state_prev must both be given or both be null (the first frame)");
    if (moments && (((uintptr_t)d_moment_prev & 15u) || ((uintptr_t)d_moment_next & 15u))) return fail(-2, "both moment planes must be 16-byte aligned");
    if (((uintptr_t)d_features & 15u) || ((uintptr_t)d_state_prev & 15u) || ((uintptr_t)d_state_next & 15u)) return fail(-2, "the feature buffer and both states must be 16-byte aligned");
    if (((uintptr_t)d_image & (sizeof(T) - 1)) || ((uintptr_t)d_out & (sizeof(T) - 1))) return fail(-2, "the image buffers must be aligned to their element type");
    const size_t n_pix = (size_t)width * (size_t)height;
    const size_t img_b = n_pix * 3 * sizeof(T), feat_b = n_pix * 8 * sizeof(T), st_b = (size_t)state_bytes(width, height, sizeof(T));
    if (ranges_overlap(d_out, img_b, d_state_next, st_b)) return fail(-2, "d_out and d_state_next may not alias each other");
    if (ranges_overlap(d_out, img_b, d_image, img_b) || ranges_overlap(d_out, img_b, d_features, feat_b) || (d_state_prev && ranges_overlap(d_out, img_b, d_state_prev, st_b)))
        return fail(-2, "d_out may not alias an input");
    if (ranges_overlap(d_state_next, st_b, d_image, img_b) || ranges_overlap(d_state_next, st_b, d_features, feat_b) || (d_state_prev && ranges_overlap(d_state_next, st_b, d_state_prev, st_b)))
        return fail(-2, "d_state_next may not alias an input");
    if (moments) {
        const size_t mo_b = (size_t)moment_bytes(width, height, sizeof(T));
        if (ranges_overlap(d_moment_next, mo_b, d_out, img_b) || ranges_overlap(d_moment_next, mo_b, d_state_next, st_b)) return fail(-2, "d_moment_next may not alias another output");
        if (ranges_overlap(d_moment_next, mo_b, d_image, img_b) || ranges_overlap(d_moment_next, mo_b, d_features, feat_b) ||
            (d_state_prev && (ranges_overlap(d_moment_next, mo_b, d_state_prev, st_b) || ranges_overlap(d_moment_next, mo_b, d_moment_prev, mo_b))))
            return fail(-2, "d_moment_next may not alias an input");
        if (d_moment_prev && (ranges_overlap(d_moment_prev, mo_b, d_out, img_b) || ranges_overlap(d_moment_prev, mo_b, d_state_next, st_b)))
            return fail(-2, "d_moment_prev may not alias an output");
    }
    DeviceGuard guard;
    if (t->device >= 0) HIP_TRY(hipSetDevice(t->device));
    return launch_temporal<T>(t, cam, cam_prev, width, height, d_image, d_features, d_state_prev, d_state_next, d_out, (hipStream_t)stream_v, moments ? d_moment_prev : nullptr,
                              moments ? d_moment_next : nullptr, clamped ? c : nullptr);
}

// The device-resident entry point of the noise map: nulls, the parameters, then the pointers' alignment and aliasing.
template <typename T>
int temporal_noise_device(const rtw_temporal_noise_t *n, int32_t width, int32_t height, const void *d_state, const void *d_moment, void *d_noise, void *stream_v) {
    if (!n || !d_state || !d_moment || !d_noise) return fail(-1, "null argument");
    if (int rc = validate_temporal_noise(n, width, height, (int)sizeof(T))) return rc;
    if (((uintptr_t)d_state & 15u) || ((uintptr_t)d_moment & 15u)) return fail(-2, "the state and the moment plane must be 16-byte aligned");
    if ((uintptr_t)d_noise & (sizeof(T) - 1)) return fail(-2, "the noise map must be aligned to its element type");
    const size_t n_pix = (size_t)width * (size_t)height;
    if (ranges_overlap(d_noise, n_pix * sizeof(T), d_state, (size_t)state_bytes(width, height, sizeof(T))) ||
        ranges_overlap(d_noise, n_pix * sizeof(T), d_moment, (size_t)moment_bytes(width, height, sizeof(T))))
        return fail(-2, "d_noise may not alias an input");
    DeviceGuard guard;
    if (n->device >= 0) HIP_TRY(hipSetDevice(n->device));
    return launch_temporal_noise<T>(n, width, height, d_state, d_moment, d_noise, (hipStream_t)stream_v);
}

}  // namespace rtwh

using namespace rtwh;

extern "C" {

int64_t rtw_temporal_state_bytes(int32_t width, int32_t height, int32_t elem_bytes) {
    if (const int64_t rc = rtw_denoise_work_bytes(width, height, elem_bytes); rc < 0) return rc;             // (elem_bytes, the sizes, the denoiser's frame rule)
    return state_bytes(width, height, elem_bytes);
}
int64_t rtw_history_moment_bytes(int32_t width, int32_t height, int32_t elem_bytes) {
    if (const int64_t rc = rtw_denoise_work_bytes(width, height, elem_bytes); rc < 0) return rc;             // (the same checks and codes)
    return moment_bytes(width, height, elem_bytes);
}
int rtw_temporal_device_f32(const rtw_temporal_t *t, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width, int32_t height, const void *d_image,
                            const void *d_features, const void *d_state_prev, void *d_state_next, void *d_out, void *hip_stream) {
    return temporal_device<float>(t, cam, cam_prev, width, height, d_image, d_features, d_state_prev, d_state_next, d_out, hip_stream);
}
int rtw_temporal_device_f64(const rtw_temporal_t *t, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width, int32_t height, const void *d_image,
                            const void *d_features, const void *d_state_prev, void *d_state_next, void *d_out, void *hip_stream) {
    return temporal_device<double>(t, cam, cam_prev, width, height, d_image, d_features, d_state_prev, d_state_next, d_out, hip_stream);
}
int rtw_history_moments_device_f32(const rtw_temporal_t *t, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width, int32_t height, const void *d_image,
                                    const void *d_features, const void *d_state_prev, const void *d_moment_prev, void *d_state_next, void *d_moment_next, void *d_out, void *hip_stream) {
    return temporal_device<float>(t, cam, cam_prev, width, height, d_image, d_features, d_state_prev, d_state_next, d_out, hip_stream, true, d_moment_prev, d_moment_next);
}
int rtw_history_moments_device_f64(const rtw_temporal_t *t, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width, int32_t height, const void *d_image,
                                    const void *d_features, const void *d_state_prev, const void *d_moment_prev, void *d_state_next, void *d_moment_next, void *d_out, void *hip_stream) {
    return temporal_device<double>(t, cam, cam_prev, width, height, d_image, d_features, d_state_prev, d_state_next, d_out, hip_stream, true, d_moment_prev, d_moment_next);
}
int rtw_clamped_step_device_f32(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width, int32_t height,
                                    const void *d_image, const void *d_features, const void *d_state_prev, const void *d_moment_prev, void *d_state_next, void *d_moment_next, void *d_out,
                                    void *hip_stream) {
    return temporal_device<float>(t, cam, cam_prev, width, height, d_image, d_features, d_state_prev, d_state_next, d_out, hip_stream, d_moment_prev || d_moment_next, d_moment_prev,
                                  d_moment_next, true, c);
}
int rtw_clamped_step_device_f64(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width, int32_t height,
                                    const void *d_image, const void *d_features, const void *d_state_prev, const void *d_moment_prev, void *d_state_next, void *d_moment_next, void *d_out,
                                    void *hip_stream) {
    return temporal_device<double>(t, cam, cam_prev, width, height, d_image, d_features, d_state_prev, d_state_next, d_out, hip_stream, d_moment_prev || d_moment_next, d_moment_prev,
                                   d_moment_next, true, c);
}
int rtw_history_noise_device_f32(const rtw_temporal_noise_t *n, int32_t width, int32_t height, const void *d_state, const void *d_moment, void *d_noise, void *hip_stream) {
    return temporal_noise_device<float>(n, width, height, d_state, d_moment, d_noise, hip_stream);
}
int rtw_history_noise_device_f64(const rtw_temporal_noise_t *n, int32_t width, int32_t height, const void *d_state, const void *d_moment, void *d_noise, void *hip_stream) {
    return temporal_noise_device<double>(n, width, height, d_state, d_moment, d_noise, hip_stream);
}

}  // extern "C"
