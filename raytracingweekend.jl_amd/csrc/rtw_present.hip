// rtw_present.hip -- the present stage (include/rtw_hip.h rtw_present_*): the checks that need no device, the one launch of its kernel
// (rtw_present.hpp) for one frame or a batch of frames and the device-resident entry points.  n_views == 0 is one frame; n_views >= 1
// (rtw_present_batch_device_*) that many frames in the same launch.
// (The host-buffer entry points live with the other cached-context paths: rtw_present_* in rtw_stage_host.hip, rtw_render_presented_* in rtw_render_host.hip.)
#include "rtw_host.hpp"
#include "rtw_present.hpp"

namespace rtwh {

static long long tiles_of(int32_t width, int32_t height) { return (long long)((height + RTW_PR_TILE - 1) / RTW_PR_TILE) * ((width + RTW_PR_TILE - 1) / RTW_PR_TILE); }

// the size of a call: a frame, channels, views (0: one frame), and no more tiles than one launch numbers
static int check_size(int32_t width, int32_t height, int32_t channels, int32_t n_views) {
    if (channels != 3 && channels != 4) return fail(-2, "channels must be 3 or 4 (got %d)", channels);
    if (width < 1 || height < 1) return fail(-2, "width/height must be positive (got %d x %d)", width, height);
    if (n_views < 0) return fail(-2, "n_views must be >= 1");
    if ((double)tiles_of(width, height) * (double)(n_views ? n_views : 1) >= (double)(1ll << 31))
        return fail(-5, "frames too large for one call: %d views of %d x %d pixels", n_views ? n_views : 1, width, height);
    return 0;
}

// Everything about a present call that is decided without a device and without a pointer.  n_views == 0: one frame; a batched entry point
// hands its count down through batch_views, so a count that is no batch arrives negative.
int validate_present(const rtw_present_t *p, int32_t width, int32_t height, int32_t n_views) {
    if (!p) return fail(-1, "null present parameters");
    if (p->flags & ~(RTW_PRESENT_DITHER | RTW_PRESENT_BGR | RTW_PRESENT_SQRT)) return fail(-2, "unknown present flags 0x%x", p->flags);
    if (p->reserved0 != 0 || p->reserved[0] != 0 || p->reserved[1] != 0) return fail(-2, "reserved must be 0");
    if (!(p->exposure > 0) || !std::isfinite(p->exposure)) return fail(-2, "exposure must be finite and positive");
    if (p->device < -1) return fail(-2, "bad device %d", p->device);
    return check_size(width, height, p->channels, n_views);
}

// Enqueue the ONE launch on `stream` of the current device (validate_present has accepted the call).
template <typename T>
int launch_present(const rtw_present_t *p, int32_t width, int32_t height, int32_t n_views, const void *d_images, void *d_out, hipStream_t stream) {
    rtw::PrParams U;
    memset(&U, 0, sizeof U);
    U.exposure = p->exposure;
    U.W = width; U.H = height;
    U.tiles_y = (height + RTW_PR_TILE - 1) / RTW_PR_TILE;
    U.tiles_per_view = (int)tiles_of(width, height);
    U.flags = p->flags;
    U.nan_rgb = (unsigned)p->nan_rgb[0] | ((unsigned)p->nan_rgb[1] << 8) | ((unsigned)p->nan_rgb[2] << 16);
    const unsigned grid = (unsigned)(tiles_of(width, height) * (n_views ? n_views : 1));
    // (measurement aid, tools/gpu_present.py: events around the kernel, reported on stderr -- this one blocks)
    static const bool profile = aid_flag("RTW_PRESENT_PROFILE");
    StageMarks marks(profile, stream);
    HIP_TRY(marks.mark());
    (void)hipGetLastError();
    const T *in = (const T *)d_images;
    unsigned char *out = (unsigned char *)d_out;
    const bool aligned = width % 4 == 0;                     // C = 3: every row of every view starts on a dword
    if (p->channels == 4) hipLaunchKernelGGL((rtw::pr_present<T, 4, true>), dim3(grid), dim3(256), 0, stream, U, in, out);
    else if (aligned) hipLaunchKernelGGL((rtw::pr_present<T, 3, true>), dim3(grid), dim3(256), 0, stream, U, in, out);
    else hipLaunchKernelGGL((rtw::pr_present<T, 3, false>), dim3(grid), dim3(256), 0, stream, U, in, out);
    HIP_TRY(hipGetLastError());
    if (profile) {
        HIP_TRY(marks.mark());
        HIP_TRY(marks.measure());
        fprintf(stderr, "[rtw present] %s %dx%d views=%d C=%d %s ms=%.5f\n", sizeof(T) == 8 ? "f64" : "f32", width, height, n_views ? n_views : 1, p->channels,
                p->channels == 4 ? "dword" : aligned ? "aligned" : "unaligned", marks.ms[0]);
    }
    return 0;
}

// The device-resident entry points: nulls, the parameters, then the pointers' alignment and aliasing over the extents of all frames.
template <typename T>
int present_device(const rtw_present_t *p, int32_t width, int32_t height, int32_t n_views, const void *d_images, void *d_out, void *stream_v) {
    if (!p || !d_images || !d_out) return fail(-1, "null argument");
    if (int rc = validate_present(p, width, height, n_views)) return rc;
    if ((uintptr_t)d_out & 3u) return fail(-2, "d_out must be 4-byte aligned");
    if ((uintptr_t)d_images & (sizeof(T) - 1)) return fail(-2, "the image buffer must be aligned to its element type");
    const size_t n_pix = (size_t)width * (size_t)height * (n_views ? (size_t)n_views : 1);
    if (ranges_overlap(d_out, n_pix * (size_t)p->channels, d_images, n_pix * 3 * sizeof(T))) return fail(-2, "d_out may not alias the input");
    DeviceGuard guard;
    if (p->device >= 0) HIP_TRY(hipSetDevice(p->device));
    return launch_present<T>(p, width, height, n_views, d_images, d_out, (hipStream_t)stream_v);
}

template int launch_present<float>(const rtw_present_t *, int32_t, int32_t, int32_t, const void *, void *, hipStream_t);
template int launch_present<double>(const rtw_present_t *, int32_t, int32_t, int32_t, const void *, void *, hipStream_t);

}  // namespace rtwh

using namespace rtwh;

extern "C" {

int64_t rtw_present_bytes(int32_t width, int32_t height, int32_t channels, int32_t n_views) {
    if (int rc = check_size(width, height, channels, n_views)) return rc;
    return (int64_t)width * height * channels * (n_views ? n_views : 1);
}
int rtw_present_device_f32(const rtw_present_t *p, int32_t width, int32_t height, const void *d_image, void *d_out, void *hip_stream) {
    return present_device<float>(p, width, height, 0, d_image, d_out, hip_stream);
}
int rtw_present_device_f64(const rtw_present_t *p, int32_t width, int32_t height, const void *d_image, void *d_out, void *hip_stream) {
    return present_device<double>(p, width, height, 0, d_image, d_out, hip_stream);
}
int rtw_present_batch_device_f32(const rtw_present_t *p, int32_t width, int32_t height, int32_t n_views, const void *d_images, void *d_out, void *hip_stream) {
    return present_device<float>(p, width, height, batch_views(n_views), d_images, d_out, hip_stream);
}
int rtw_present_batch_device_f64(const rtw_present_t *p, int32_t width, int32_t height, int32_t n_views, const void *d_images, void *d_out, void *hip_stream) {
    return present_device<double>(p, width, height, batch_views(n_views), d_images, d_out, hip_stream);
}

}  // extern "C"
