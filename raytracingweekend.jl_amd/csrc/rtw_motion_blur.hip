// rtw_motion_blur.hip -- the motion-blur stage (include/rtw_hip.h rtw_velocity_blur_*): the checks that need no device, the workspace's layout,
// the three launches of its kernels (rtw_motion_blur.hpp) and the device-resident entry points.
// (The host-buffer entry points live with the other cached-context paths: rtw_velocity_blur_* in rtw_stage_host.hip, rtw_render_blurred_* in
// rtw_render_host.hip.)
#include "rtw_host.hpp"
#include "rtw_motion_blur.hpp"

namespace rtwh {

// Everything about a blur that is decided without a device and without a pointer.
int validate_motion_blur(const rtw_velocity_blur_t *b, int32_t width, int32_t height, int elem_bytes) {
    if (!b) return fail(-1, "null motion blur parameters");
    if (b->taps < 3 || b->taps > 31 || !(b->taps & 1)) return fail(-2, "taps must be odd and in 3..31 (got %d)", b->taps);
    if (b->flags != 0) return fail(-2, "unknown motion blur flags 0x%x", b->flags);
    if (b->gamma != 0 && b->gamma != 1) return fail(-2, "gamma must be 0 or 1 (got %d)", b->gamma);
    if (b->device < -1) return fail(-2, "bad device %d", b->device);
    if (b->reserved[0] != 0 || b->reserved[1] != 0) return fail(-2, "reserved must be 0");
    if (!(b->shutter > 0) || !(b->shutter <= 1)) return fail(-2, "shutter must be in (0, 1]");
    if (!(b->depth_extent > 0) || !std::isfinite(b->depth_extent)) return fail(-2, "depth_extent must be finite and positive");
    if (width < 1 || height < 1) return fail(-2, "width/height must be positive (got %d x %d)", width, height);
    if (const int64_t rc = rtw_denoise_work_bytes(width, height, elem_bytes); rc < 0) return (int)rc;         // (the denoiser's frame rule)
    return 0;
}

// the workspace: the blur plane (a 4-element slot per pixel), the tile plane and the neighbour plane (a 4-element slot per tile each)
static long long tiles_of(int32_t width, int32_t height) {
    return (long long)((height + rtw::MB_TILE - 1) / rtw::MB_TILE) * ((width + rtw::MB_TILE - 1) / rtw::MB_TILE);
}
static long long work_bytes(int32_t width, int32_t height, int elem_bytes) { return ((long long)width * height + 2 * tiles_of(width, height)) * 4 * elem_bytes; }

// Enqueue the stage on `stream` of the current device (validate_motion_blur has accepted the call): THREE launches, no record.
// cam_prev null (internal: frame 0 of rtw_render_blurred_*): ONE launch of the pass-through instance -- the image's validity and
// the gamma; d_motion and d_work are not looked at.
template <typename T, typename CamT>
int launch_motion_blur(const rtw_velocity_blur_t *b, const CamT *cam, const CamT *cam_prev, int32_t width, int32_t height, const void *d_image, const void *d_features,
                       const void *d_motion, void *d_work, void *d_out, hipStream_t stream) {
    using V = typename rtw::DnVec<T>::type;
    const int TH = (height + rtw::MB_TILE - 1) / rtw::MB_TILE, TW = (width + rtw::MB_TILE - 1) / rtw::MB_TILE;
    const unsigned tiles = (unsigned)tiles_of(width, height);                 // (fewer than the frame rule's 8 x 8 ones: one 32-bit grid dimension holds them)
    const T ext = (T)b->depth_extent;
    // (measurement aid, tools/gpu_motion_blur.py: events around every launch, reported on stderr -- this one blocks)
    static const bool profile = aid_flag("RTW_TEMPORAL_PROFILE");
    StageMarks marks(profile, stream);
    HIP_TRY(marks.mark());
    (void)hipGetLastError();
    if (!cam_prev) {
        hipLaunchKernelGGL((rtw::mb_gather<T, true>), dim3(tiles), dim3(256), 0, stream, width, height, b->taps, b->gamma, ext, (const T *)d_image, (const V *)d_features,
                           (const V *)nullptr, (const V *)nullptr, (T *)d_out);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    rtw::TpParams<T> U;
    memset(&U, 0, sizeof U);
    {
        T e[32];
        temporal_table<T>(cam, cam_prev, 1, e);
        memcpy(&U, e, 29 * sizeof(T));
    }
    U.W = width; U.H = height;
    V *blur = (V *)d_work, *tile = blur + (size_t)width * (size_t)height, *nb = tile + tiles;
    hipLaunchKernelGGL((rtw::mb_velocity<T>), dim3(tiles), dim3(256), 0, stream, U, (T)(b->shutter / 2), (const T *)d_image, (const V *)d_features, (const V *)d_motion, blur, tile);
    HIP_TRY(hipGetLastError());
    HIP_TRY(marks.mark());
    hipLaunchKernelGGL((rtw::mb_neighbour<T>), dim3((tiles + 255) / 256), dim3(256), 0, stream, TH, TW, (const V *)tile, nb);
    HIP_TRY(hipGetLastError());
    HIP_TRY(marks.mark());
    hipLaunchKernelGGL((rtw::mb_gather<T, false>), dim3(tiles), dim3(256), 0, stream, width, height, b->taps, b->gamma, ext, (const T *)d_image, (const V *)nullptr, (const V *)blur,
                       (const V *)nb, (T *)d_out);
    HIP_TRY(hipGetLastError());
    if (profile) {
        const float *ms = marks.ms;
        HIP_TRY(marks.mark());
        HIP_TRY(marks.measure());
        fprintf(stderr, "[rtw motion blur] %s %dx%d taps=%d velocity_ms=%.5f neighbour_ms=%.5f gather_ms=%.5f\n", sizeof(T) == 8 ? "f64" : "f32", width, height, b->taps, ms[0], ms[1], ms[2]);
    }
    return 0;
}

// The device-resident entry point: nulls, the parameters, then the pointers' alignment and aliasing.
template <typename T, typename CamT>
int motion_blur_device(const rtw_velocity_blur_t *b, const CamT *cam, const CamT *cam_prev, int32_t width, int32_t height, const void *d_image, const void *d_features, const void *d_motion,
                       void *d_work, void *d_out, void *stream_v) {
    if (!b || !cam || !cam_prev || !d_image || !d_features || !d_motion || !d_work || !d_out) return fail(-1, "null argument");
    if (int rc = validate_motion_blur(b, width, height, (int)sizeof(T))) return rc;
    if (((uintptr_t)d_features & 15u) || ((uintptr_t)d_motion & 15u) || ((uintptr_t)d_work & 15u)) return fail(-2, "the feature buffer, the motion plane and the workspace must be 16-byte aligned");
    if (((uintptr_t)d_image & (sizeof(T) - 1)) || ((uintptr_t)d_out & (sizeof(T) - 1))) return fail(-2, "the image buffers must be aligned to their element type");
    const size_t n_pix = (size_t)width * (size_t)height;
    const size_t img_b = n_pix * 3 * sizeof(T), feat_b = n_pix * 8 * sizeof(T), mo_b = n_pix * 4 * sizeof(T), work_b = (size_t)work_bytes(width, height, sizeof(T));
    if (int rc = check_alias({{"d_out", d_out, img_b}, {"d_work", d_work, work_b}}, {{"d_image", d_image, img_b}, {"d_features", d_features, feat_b}, {"d_motion", d_motion, mo_b}})) return rc;
    DeviceGuard guard;
    if (b->device >= 0) HIP_TRY(hipSetDevice(b->device));
    return launch_motion_blur<T>(b, cam, cam_prev, width, height, d_image, d_features, d_motion, d_work, d_out, (hipStream_t)stream_v);
}

template int launch_motion_blur<float>(const rtw_velocity_blur_t *, const rtw_camera_f32 *, const rtw_camera_f32 *, int32_t, int32_t, const void *, const void *, const void *, void *, void *, hipStream_t);
template int launch_motion_blur<double>(const rtw_velocity_blur_t *, const rtw_camera_f64 *, const rtw_camera_f64 *, int32_t, int32_t, const void *, const void *, const void *, void *, void *, hipStream_t);

}  // namespace rtwh

using namespace rtwh;

extern "C" {

int64_t rtw_velocity_blur_work_bytes(int32_t width, int32_t height, int32_t elem_bytes) {
    if (const int64_t rc = rtw_denoise_work_bytes(width, height, elem_bytes); rc < 0) return rc;             // (elem_bytes, the sizes, the denoiser's frame rule)
    return work_bytes(width, height, elem_bytes);
}
int rtw_velocity_blur_device_f32(const rtw_velocity_blur_t *b, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width, int32_t height, const void *d_image,
                               const void *d_features, const void *d_motion, void *d_work, void *d_out, void *hip_stream) {
    return motion_blur_device<float>(b, cam, cam_prev, width, height, d_image, d_features, d_motion, d_work, d_out, hip_stream);
}
int rtw_velocity_blur_device_f64(const rtw_velocity_blur_t *b, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width, int32_t height, const void *d_image,
                               const void *d_features, const void *d_motion, void *d_work, void *d_out, void *hip_stream) {
    return motion_blur_device<double>(b, cam, cam_prev, width, height, d_image, d_features, d_motion, d_work, d_out, hip_stream);
}

}  // extern "C"
