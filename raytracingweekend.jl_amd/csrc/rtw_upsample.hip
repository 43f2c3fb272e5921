// rtw_upsample.hip -- the feature-guided upsampler (include/rtw_hip.h rtw_upsample_*): the checks that need no device, the launch sequence --
// the denoiser's prepare and `levels` of its level kernel at the small size (rtw_denoise.hpp, launched as they are; no pass is a final one),
// then the upsampling kernel (rtw_upsample.hpp) at the full size -- and the device-resident entry points.  n_views == 0 is one frame;
// n_views >= 1 (rtw_upsample_batch_*) the same sequence once for that many views (the batched kernels).
// (The host-buffer entry points live with the other cached-context paths: rtw_upsample_* and rtw_upsample_batch_* in rtw_stage_host.hip, rtw_render_upsampled_* and rtw_render_upsampled_batch_* in rtw_render_host.hip.)
#include "rtw_host.hpp"
#include "rtw_upsample.hpp"

namespace rtwh {

// Everything about an upsampler call that is decided without a device.  n_views == 0: one frame.
int validate_upsample(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, int32_t n_views, int elem_bytes) {
    if (!u) return fail(-1, "null upsampler parameters");
    if (u->levels < 0 || u->levels > 8) return fail(-2, "levels must be in 0..8 (got %d)", u->levels);
    if (u->normal_power_log2 < 0 || u->normal_power_log2 > 7) return fail(-2, "normal_power_log2 must be in 0..7 (got %d)", u->normal_power_log2);
    if (u->flags & ~(RTW_UPSAMPLE_DEMODULATE)) return fail(-2, "unknown upsampler flags 0x%x", u->flags);
    if (u->gamma != 0 && u->gamma != 1) return fail(-2, "gamma must be 0 or 1 (got %d)", u->gamma);
    if (u->device < -1) return fail(-2, "bad device %d", u->device);
    if (u->hi_chunks < 0) return fail(-2, "hi_chunks must be >= 0 (got %d)", u->hi_chunks);
    if (!(u->sigma_color > 0) || !std::isfinite(u->sigma_color)) return fail(-2, "sigma_color must be finite and positive");
    if (!(u->sigma_depth > 0) || !std::isfinite(u->sigma_depth)) return fail(-2, "sigma_depth must be finite and positive");
    if (!(u->sigma_albedo > 0) || !std::isfinite(u->sigma_albedo)) return fail(-2, "sigma_albedo must be finite and positive");
    if (lo_width < 1 || lo_height < 1 || width < 1 || height < 1)
        return fail(-2, "widths and heights must be positive (got %d x %d -> %d x %d)", lo_width, lo_height, width, height);
    if (lo_width > width || lo_height > height)
        return fail(-2, "the small frame may not exceed the full one (got %d x %d -> %d x %d)", lo_width, lo_height, width, height);
    if (const int64_t rc = rtw_denoise_work_bytes(width, height, elem_bytes); rc < 0) return (int)rc;         // (the denoiser's frame rule, for the larger frame)
    if (n_views) {
        if (n_views < 1) return fail(-2, "n_views must be >= 1");
        if ((double)width * (double)height * (double)n_views >= (double)(1ll << 39)) return fail(-5, "batch too large for one call: %d views of %d x %d pixels", n_views, width, height);
    }
    return 0;
}

// Enqueue the upsampler on `stream` of the current device (validate_upsample has accepted the call).  The workspace is the denoiser's for the
// small frame (times n_views, batch-major: E, E', G, A with view v at slot offset v*w*h).
template <typename T>
int launch_upsample(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, int n_views, const void *d_image_lo, const void *d_features_lo,
                    const void *d_features_hi, void *d_out, void *d_work, hipStream_t stream) {
    using V = typename rtw::DnVec<T>::type;
    const bool batch = n_views != 0;
    const long long frames = batch ? n_views : 1, n_lo = (long long)lo_width * lo_height * frames, n_hi = (long long)width * height * frames;
    const long long pb = n_lo * 4 * (long long)sizeof(T);
    char *w = (char *)d_work;
    V *E[2] = {(V *)w, (V *)(w + pb)};
    V *G = (V *)(w + 2 * pb), *A = (V *)(w + 3 * pb);
    const bool demod = (u->flags & RTW_UPSAMPLE_DEMODULATE) != 0;
    const unsigned grid_lo = (unsigned)((n_lo + 255) / 256), grid_hi = (unsigned)((n_hi + 255) / 256);
    // (measurement aid, tools/gpu_upsample.py: events around every kernel, reported on stderr -- this one blocks)
    static const bool profile = aid_flag("RTW_DENOISE_PROFILE");
    StageMarks marks(profile, stream);                 // before prepare, behind prepare, behind every level, behind the upsampling
    HIP_TRY(marks.mark());
    (void)hipGetLastError();
    hipLaunchKernelGGL((rtw::dn_prepare<T, false>), dim3(grid_lo), dim3(256), 0, stream, (const T *)d_image_lo, (const V *)d_features_lo, E[0], G, A, n_lo, demod ? 1 : 0, (const T *)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(marks.mark());
    const T inv_sz = (T)(1.0 / (u->sigma_depth * u->sigma_depth));
    for (int k = 0; k < u->levels; ++k) {
        rtw::DnLevel<T> L;
        const double sc = u->sigma_color * std::ldexp(1.0, -k);
        L.inv_sc = (T)(1.0 / (sc * sc));
        L.inv_sz = inv_sz;
        L.step = 1 << k; L.m = u->normal_power_log2;
        L.mode = 0;                                    // never the final pass: the colour stays demodulated and linear in the next E plane
        L.W = lo_width; L.H = lo_height;
        const V *in = E[k & 1];
        V *next = E[(k & 1) ^ 1];
        if (batch) {
            rtw::DnLevelBatch<T> LB;
            LB.L = L; LB.n_all = n_lo;
            hipLaunchKernelGGL((rtw::dn_level_batch<T, false>), dim3(grid_lo), dim3(256), 0, stream, LB, in, (const V *)G, (const V *)A, next, (T *)nullptr);
        } else hipLaunchKernelGGL((rtw::dn_level<T, false>), dim3(grid_lo), dim3(256), 0, stream, L, in, (const V *)G, (const V *)A, next, (T *)nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(marks.mark());
    }
    rtw::UpParamsBatch<T> B;
    B.U.inv_sa = (T)(1.0 / (u->sigma_albedo * u->sigma_albedo));
    B.U.inv_sz = inv_sz;
    B.U.m = u->normal_power_log2;
    B.U.mode = (demod ? RTW_DN_DEMOD : 0) | (u->gamma ? RTW_DN_GAMMA : 0);
    B.U.w = lo_width; B.U.h = lo_height; B.U.W = width; B.U.H = height;
    B.n_all = n_hi;
    const V *Ef = E[u->levels & 1];
    if (batch) hipLaunchKernelGGL((rtw::up_sample<T, true>), dim3(grid_hi), dim3(256), 0, stream, B, Ef, (const V *)G, (const V *)A, (const V *)d_features_hi, (T *)d_out);
    else hipLaunchKernelGGL((rtw::up_sample<T, false>), dim3(grid_hi), dim3(256), 0, stream, B, Ef, (const V *)G, (const V *)A, (const V *)d_features_hi, (T *)d_out);
    HIP_TRY(hipGetLastError());
    if (profile) {
        HIP_TRY(marks.mark());
        const char *ts = sizeof(T) == 8 ? "f64" : "f32";
        char size[96];                                                          // (a batch: " views=N" behind the sizes)
        if (batch) snprintf(size, sizeof size, "%dx%d->%dx%d views=%d", lo_width, lo_height, width, height, n_views);
        else snprintf(size, sizeof size, "%dx%d->%dx%d", lo_width, lo_height, width, height);
        HIP_TRY(marks.measure());
        for (int k = 0; k + 1 < marks.n; ++k) {
            if (k == 0) fprintf(stderr, "[rtw upsample] %s %s prepare ms=%.5f\n", ts, size, marks.ms[k]);
            else if (k <= u->levels) fprintf(stderr, "[rtw upsample] %s %s level step=%d ms=%.5f\n", ts, size, 1 << (k - 1), marks.ms[k]);
            else fprintf(stderr, "[rtw upsample] %s %s upsample ms=%.5f\n", ts, size, marks.ms[k]);
        }
        fprintf(stderr, "[rtw upsample] %s %s total levels=%d ms=%.5f\n", ts, size, u->levels, marks.total_ms);
    }
    return 0;
}

// The device-resident entry points.  n_views == 0: rtw_upsample_device_*; n_views != 0: rtw_upsample_batch_device_*.  The alignment and aliasing
// checks cover the extents of all frames.
template <typename T>
int upsample_device(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, int32_t n_views, const void *d_image_lo, const void *d_features_lo,
                    const void *d_features_hi, void *d_out, void *d_work, void *stream_v) {
    if (!u || !d_image_lo || !d_features_lo || !d_features_hi || !d_out || !d_work) return fail(-1, "null argument");
    if (int rc = validate_upsample(u, lo_width, lo_height, width, height, n_views, (int)sizeof(T))) return rc;
    if (((uintptr_t)d_work & 15u) || ((uintptr_t)d_features_lo & 15u) || ((uintptr_t)d_features_hi & 15u)) return fail(-2, "the workspace and the feature buffers must be 16-byte aligned");
    if (((uintptr_t)d_image_lo & (sizeof(T) - 1)) || ((uintptr_t)d_out & (sizeof(T) - 1))) return fail(-2, "the image buffers must be aligned to their element type");
    const size_t frames = n_views ? (size_t)n_views : 1, n_lo = (size_t)lo_width * (size_t)lo_height * frames, n_hi = (size_t)width * (size_t)height * frames;
    const size_t img_b = n_lo * 3 * sizeof(T), flo_b = n_lo * 8 * sizeof(T), fhi_b = n_hi * 8 * sizeof(T), out_b = n_hi * 3 * sizeof(T), work_b = n_lo * 16 * sizeof(T);
    if (ranges_overlap(d_out, out_b, d_image_lo, img_b) || ranges_overlap(d_out, out_b, d_features_lo, flo_b) || ranges_overlap(d_out, out_b, d_features_hi, fhi_b) ||
        ranges_overlap(d_out, out_b, d_work, work_b))
        return fail(-2, "d_out may not alias an input or the workspace");
    if (ranges_overlap(d_work, work_b, d_image_lo, img_b) || ranges_overlap(d_work, work_b, d_features_lo, flo_b) || ranges_overlap(d_work, work_b, d_features_hi, fhi_b))
        return fail(-2, "the workspace may not alias an input");
    DeviceGuard guard;
    if (u->device >= 0) HIP_TRY(hipSetDevice(u->device));
    return launch_upsample<T>(u, lo_width, lo_height, width, height, n_views, d_image_lo, d_features_lo, d_features_hi, d_out, d_work, (hipStream_t)stream_v);
}

template int launch_upsample<float>(const rtw_upsample_t *, int32_t, int32_t, int32_t, int32_t, int32_t, const void *, const void *, const void *, void *, void *, hipStream_t);
template int launch_upsample<double>(const rtw_upsample_t *, int32_t, int32_t, int32_t, int32_t, int32_t, const void *, const void *, const void *, void *, void *, hipStream_t);

}  // namespace rtwh

using namespace rtwh;

extern "C" {

int64_t rtw_upsample_work_bytes(int32_t lo_width, int32_t lo_height, int32_t elem_bytes) { return rtw_denoise_work_bytes(lo_width, lo_height, elem_bytes); }
int rtw_upsample_device_f32(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, const void *d_image_lo, const void *d_features_lo,
                            const void *d_features_hi, void *d_out, void *d_work, void *hip_stream) {
    return upsample_device<float>(u, lo_width, lo_height, width, height, 0, d_image_lo, d_features_lo, d_features_hi, d_out, d_work, hip_stream);
}
int rtw_upsample_device_f64(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, const void *d_image_lo, const void *d_features_lo,
                            const void *d_features_hi, void *d_out, void *d_work, void *hip_stream) {
    return upsample_device<double>(u, lo_width, lo_height, width, height, 0, d_image_lo, d_features_lo, d_features_hi, d_out, d_work, hip_stream);
}
int rtw_upsample_batch_device_f32(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, int32_t n_views, const void *d_images_lo,
                                  const void *d_features_lo, const void *d_features_hi, void *d_out, void *d_work, void *hip_stream) {
    return upsample_device<float>(u, lo_width, lo_height, width, height, batch_views(n_views), d_images_lo, d_features_lo, d_features_hi, d_out, d_work, hip_stream);
}
int rtw_upsample_batch_device_f64(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, int32_t n_views, const void *d_images_lo,
                                  const void *d_features_lo, const void *d_features_hi, void *d_out, void *d_work, void *hip_stream) {
    return upsample_device<double>(u, lo_width, lo_height, width, height, batch_views(n_views), d_images_lo, d_features_lo, d_features_hi, d_out, d_work, hip_stream);
}

}  // extern "C"
