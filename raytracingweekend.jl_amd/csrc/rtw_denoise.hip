// rtw_denoise.hip -- the feature-guided denoiser (include/rtw_hip.h rtw_denoise_*): the checks that need no device, the launch sequence of
// its kernels (rtw_denoise.hpp: prepare, then the level kernel once per a-trous pass, the last one writing the image) and the device-resident
// entry points.  n_views == 0 is one frame; n_views >= 1 (rtw_filter_batch_*) the same sequence once for that many frames (the batched level
// kernel).  (The host-buffer entry points live with the other cached-context paths: rtw_denoise_* and rtw_filter_batch_* in rtw_stage_host.hip, rtw_render_denoised_* and rtw_render_filtered_batch_* in rtw_render_host.hip.)
#include "rtw_host.hpp"
#include "rtw_denoise.hpp"

namespace rtwh {

// the frame of a denoiser call: a size, and no more tiles than the feature pass numbers (validate_features)
static int check_frame(int32_t width, int32_t height) {
    if (width < 1 || height < 1) return fail(-2, "width/height must be positive (got %d x %d)", width, height);
    const long long n_tiles = (long long)((height + 7) / 8) * ((width + 7) / 8);
    if (n_tiles >= (1ll << 31)) return fail(-5, "frame too large for one call: %lld tiles", n_tiles);
    return 0;
}

// Everything about a denoiser call that is decided without a device.
int validate_denoise(const rtw_denoise_t *d, int32_t width, int32_t height) {
    if (!d) return fail(-1, "null denoiser parameters");
    if (d->levels < 1 || d->levels > 8) return fail(-2, "levels must be in 1..8 (got %d)", d->levels);
    if (d->normal_power_log2 < 0 || d->normal_power_log2 > 7) return fail(-2, "normal_power_log2 must be in 0..7 (got %d)", d->normal_power_log2);
    if (d->flags & ~(RTW_DENOISE_DEMODULATE)) return fail(-2, "unknown denoiser flags 0x%x", d->flags);
    if (d->gamma != 0 && d->gamma != 1) return fail(-2, "gamma must be 0 or 1 (got %d)", d->gamma);
    if (d->reserved != 0) return fail(-2, "reserved must be 0");
    if (d->device < -1) return fail(-2, "bad device %d", d->device);
    if (!(d->sigma_color > 0) || !std::isfinite(d->sigma_color)) return fail(-2, "sigma_color must be finite and positive");
    if (!(d->sigma_depth > 0) || !std::isfinite(d->sigma_depth)) return fail(-2, "sigma_depth must be finite and positive");
    return check_frame(width, height);
}

// the workspace: the planes E, E', G and A of rtw_denoise.hpp, 4 elements per pixel each
static long long plane_bytes(int32_t width, int32_t height, int elem_bytes) { return (long long)width * height * 4 * elem_bytes; }

// Enqueue the denoiser on `stream` of the current device (validate_denoise has accepted the call).  d_noise non-null: the noise-guided
// form -- the GUIDED instances of both kernels, the same launch sequence and workspace (the variance lives in the A plane's fourth slot).
// n_views >= 1 (rtw_filter_batch_*, rtw_guided_filter_batch_device_*; validate_filter_batch has accepted it): the same sequence ONCE for n_views frames --
// every buffer and every plane of the workspace holds the views one behind the other, so prepare (which looks at its own pixel only) runs
// over all N*W*H pixels (the guided one with a noise map of N*W*H elements) and the level kernel is the batched one, which bounds the taps by
// each view's own frame.  n_views == 0: one frame.
template <typename T>
int launch_denoise(const rtw_denoise_t *d, int32_t width, int32_t height, int n_views, const void *d_image, const void *d_features, void *d_out, void *d_work, hipStream_t stream,
                   const void *d_noise) {
    using V = typename rtw::DnVec<T>::type;
    const bool batch = n_views != 0;
    const long long frames = batch ? n_views : 1, n_pix = (long long)width * height * frames, pb = plane_bytes(width, height, sizeof(T)) * frames;
    char *w = (char *)d_work;
    V *E[2] = {(V *)w, (V *)(w + pb)};
    V *G = (V *)(w + 2 * pb), *A = (V *)(w + 3 * pb);
    const bool demod = (d->flags & RTW_DENOISE_DEMODULATE) != 0;
    const unsigned grid = (unsigned)((n_pix + 255) / 256);
    // (measurement aid, tools/gpu_denoise.py: events around every kernel, reported on stderr -- this one blocks)
    static const bool profile = aid_flag("RTW_DENOISE_PROFILE");
    StageMarks marks(profile, stream);
    HIP_TRY(marks.mark());
    (void)hipGetLastError();
    const bool guided = d_noise != nullptr;
    if (guided) hipLaunchKernelGGL((rtw::dn_prepare<T, true>), dim3(grid), dim3(256), 0, stream, (const T *)d_image, (const V *)d_features, E[0], G, A, n_pix, demod ? 1 : 0, (const T *)d_noise);
    else hipLaunchKernelGGL((rtw::dn_prepare<T, false>), dim3(grid), dim3(256), 0, stream, (const T *)d_image, (const V *)d_features, E[0], G, A, n_pix, demod ? 1 : 0, (const T *)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(marks.mark());
    for (int k = 0; k < d->levels; ++k) {
        rtw::DnLevel<T> L;
        const double sc = d->sigma_color * std::ldexp(1.0, -k);
        L.inv_sc = (T)(1.0 / (sc * sc));
        L.inv_sz = (T)(1.0 / (d->sigma_depth * d->sigma_depth));
        L.step = 1 << k; L.m = d->normal_power_log2;
        L.mode = k == d->levels - 1 ? (RTW_DN_FINAL | (demod ? RTW_DN_DEMOD : 0) | (d->gamma ? RTW_DN_GAMMA : 0)) : 0;
        L.W = width; L.H = height;
        const V *in = E[k & 1];
        V *next = E[(k & 1) ^ 1];
        if (batch) {
            rtw::DnLevelBatch<T> LB;
            LB.L = L; LB.n_all = n_pix;
            if (guided) hipLaunchKernelGGL((rtw::dn_level_batch<T, true>), dim3(grid), dim3(256), 0, stream, LB, in, (const V *)G, (const V *)A, next, (T *)d_out);
            else hipLaunchKernelGGL((rtw::dn_level_batch<T, false>), dim3(grid), dim3(256), 0, stream, LB, in, (const V *)G, (const V *)A, next, (T *)d_out);
        } else if (guided) hipLaunchKernelGGL((rtw::dn_level<T, true>), dim3(grid), dim3(256), 0, stream, L, in, (const V *)G, (const V *)A, next, (T *)d_out);
        else hipLaunchKernelGGL((rtw::dn_level<T, false>), dim3(grid), dim3(256), 0, stream, L, in, (const V *)G, (const V *)A, next, (T *)d_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(marks.mark());
    }
    if (profile) {
        const char *tag = guided ? "rtw denoise guided" : "rtw denoise";       // (tools/gpu_accum_denoise.py tells the two forms apart by it)
        char views[32] = "";                                                    // (a batched filter: " views=N" behind the frame's size)
        if (batch) snprintf(views, sizeof views, " views=%d", n_views);
        HIP_TRY(marks.measure());
        for (int k = 0; k <= d->levels; ++k) {
            if (k == 0) fprintf(stderr, "[%s] %s %dx%d%s prepare ms=%.5f\n", tag, sizeof(T) == 8 ? "f64" : "f32", width, height, views, marks.ms[k]);
            else fprintf(stderr, "[%s] %s %dx%d%s level step=%d final=%d ms=%.5f\n", tag, sizeof(T) == 8 ? "f64" : "f32", width, height, views, 1 << (k - 1),
                         (int)(k == d->levels), marks.ms[k]);
        }
        fprintf(stderr, "[%s] %s %dx%d%s total levels=%d ms=%.5f\n", tag, sizeof(T) == 8 ? "f64" : "f32", width, height, views, d->levels, marks.total_ms);
    }
    return 0;
}

// A batched filter call (rtw_filter_batch_*): validate_denoise for the frame, and a batch whose pixels the launches can number (256 per workgroup)
int validate_filter_batch(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views) {
    if (int rc = validate_denoise(d, width, height)) return rc;
    if (n_views < 1) return fail(-2, "n_views must be >= 1");
    if ((double)width * (double)height * (double)n_views >= (double)(1ll << 39)) return fail(-5, "batch too large for one call: %d views of %d x %d pixels", n_views, width, height);
    return 0;
}

// The device-resident entry points.  n_views == 0: one frame, rtw_denoise_device_* or, with d_noise (H*W elements of T), rtw_guided_filter_device_*;
// n_views != 0: rtw_filter_batch_device_* or, with d_noise (n_views*H*W elements), rtw_guided_filter_batch_device_*.  The alignment and aliasing checks cover the extents of all frames.
template <typename T>
int denoise_device(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views, const void *d_image, const void *d_features, const void *d_noise, bool guided, void *d_out,
                   void *d_work, void *stream_v) {
    if (!d || !d_image || !d_features || !d_out || !d_work || (guided && !d_noise)) return fail(-1, "null argument");
    if (int rc = n_views ? validate_filter_batch(d, width, height, n_views) : validate_denoise(d, width, height)) return rc;
    if (((uintptr_t)d_work & 15u) || ((uintptr_t)d_features & 15u)) return fail(-2, "the workspace and the feature buffer must be 16-byte aligned");
    if (((uintptr_t)d_image & (sizeof(T) - 1)) || ((uintptr_t)d_out & (sizeof(T) - 1))) return fail(-2, "the image buffers must be aligned to their element type");
    const size_t frames = n_views ? (size_t)n_views : 1, n_pix = (size_t)width * (size_t)height * frames;
    const size_t img_b = n_pix * 3 * sizeof(T), feat_b = n_pix * 8 * sizeof(T), noise_b = n_pix * sizeof(T), work_b = 4 * (size_t)plane_bytes(width, height, sizeof(T)) * frames;
    if (ranges_overlap(d_out, img_b, d_image, img_b) || ranges_overlap(d_out, img_b, d_features, feat_b) || ranges_overlap(d_out, img_b, d_work, work_b))
        return fail(-2, "d_out may not alias an input or the workspace");
    if (ranges_overlap(d_work, work_b, d_image, img_b) || ranges_overlap(d_work, work_b, d_features, feat_b)) return fail(-2, "the workspace may not alias an input");
    if (guided) {
        if ((uintptr_t)d_noise & (sizeof(T) - 1)) return fail(-2, "the noise map must be aligned to its element type");
        if (ranges_overlap(d_out, img_b, d_noise, noise_b)) return fail(-2, "d_out may not alias an input or the workspace");
        if (ranges_overlap(d_work, work_b, d_noise, noise_b)) return fail(-2, "the workspace may not alias an input");
    }
    DeviceGuard guard;
    if (d->device >= 0) HIP_TRY(hipSetDevice(d->device));
    return launch_denoise<T>(d, width, height, n_views, d_image, d_features, d_out, d_work, (hipStream_t)stream_v, guided ? d_noise : nullptr);
}

template int launch_denoise<float>(const rtw_denoise_t *, int32_t, int32_t, int32_t, const void *, const void *, void *, void *, hipStream_t, const void *);
template int launch_denoise<double>(const rtw_denoise_t *, int32_t, int32_t, int32_t, const void *, const void *, void *, void *, hipStream_t, const void *);

}  // namespace rtwh

using namespace rtwh;

extern "C" {

int64_t rtw_denoise_work_bytes(int32_t width, int32_t height, int32_t elem_bytes) {
    if (elem_bytes != 4 && elem_bytes != 8) return fail(-2, "elem_bytes must be 4 or 8 (got %d)", elem_bytes);
    if (int rc = check_frame(width, height)) return rc;
    return 4 * plane_bytes(width, height, elem_bytes);
}
int rtw_denoise_device_f32(const rtw_denoise_t *d, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_out, void *d_work, void *hip_stream) {
    return denoise_device<float>(d, width, height, 0, d_image, d_features, nullptr, false, d_out, d_work, hip_stream);
}
int rtw_denoise_device_f64(const rtw_denoise_t *d, int32_t width, int32_t height, const void *d_image, const void *d_features, void *d_out, void *d_work, void *hip_stream) {
    return denoise_device<double>(d, width, height, 0, d_image, d_features, nullptr, false, d_out, d_work, hip_stream);
}
int rtw_guided_filter_device_f32(const rtw_denoise_t *d, int32_t width, int32_t height, const void *d_image, const void *d_features, const void *d_noise, void *d_out, void *d_work,
                                 void *hip_stream) {
    return denoise_device<float>(d, width, height, 0, d_image, d_features, d_noise, true, d_out, d_work, hip_stream);
}
int rtw_guided_filter_device_f64(const rtw_denoise_t *d, int32_t width, int32_t height, const void *d_image, const void *d_features, const void *d_noise, void *d_out, void *d_work,
                                 void *hip_stream) {
    return denoise_device<double>(d, width, height, 0, d_image, d_features, d_noise, true, d_out, d_work, hip_stream);
}
int rtw_filter_batch_device_f32(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views, const void *d_images, const void *d_features, void *d_out, void *d_work,
                                void *hip_stream) {
    return denoise_device<float>(d, width, height, batch_views(n_views), d_images, d_features, nullptr, false, d_out, d_work, hip_stream);
}
int rtw_filter_batch_device_f64(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views, const void *d_images, const void *d_features, void *d_out, void *d_work,
                                void *hip_stream) {
    return denoise_device<double>(d, width, height, batch_views(n_views), d_images, d_features, nullptr, false, d_out, d_work, hip_stream);
}
int rtw_guided_filter_batch_device_f32(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views, const void *d_images, const void *d_features, const void *d_noise,
                                       void *d_out, void *d_work, void *hip_stream) {
    return denoise_device<float>(d, width, height, batch_views(n_views), d_images, d_features, d_noise, true, d_out, d_work, hip_stream);
}
int rtw_guided_filter_batch_device_f64(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views, const void *d_images, const void *d_features, const void *d_noise,
                                       void *d_out, void *d_work, void *hip_stream) {
    return denoise_device<double>(d, width, height, batch_views(n_views), d_images, d_features, d_noise, true, d_out, d_work, hip_stream);
}

}  // extern "C"
