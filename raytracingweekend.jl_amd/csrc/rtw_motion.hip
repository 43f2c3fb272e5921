// rtw_motion.hip -- the first-hit motion pass (include/rtw_hip.h rtw_first_hit_motion_*, rtw_motion_table_*): the checks that need no device,
// the motion table (pure host code), the one launch of the pass's kernel (rtw_motion.hpp) and the device-resident entry points.
// (The step that reads the plane, rtw_animated_step_device_*, lives with the other steps in rtw_temporal.hip; the host-buffer entry points
// live with the other cached-context paths: rtw_first_hit_motion_* in rtw_render_host.hip, rtw_animated_step_* in rtw_stage_host.hip.)
#include "rtw_scene_view.hpp"
#include "rtw_motion.hpp"

namespace rtwh {

// Everything about a motion pass that is decided without a device and without a pointer: of `p` the frame, the device and the flag bits are
// read (the scan-mode flags are accepted and change nothing; spp, depth, seed and chunks are not looked at).
int validate_motion(const rtw_params *p, int elem_bytes) {
    if (!p) return fail(-1, "null params");
    if (p->width < 1 || p->height < 1) return fail(-2, "width/height must be positive (got %d x %d)", p->width, p->height);
    if (p->device < -1) return fail(-2, "bad device %d", p->device);
    if (p->flags & ~(RTW_FLAG_GROUP_CULL | RTW_FLAG_SCAN_VALU | RTW_FLAG_NUMERICS_CONTRACT | RTW_FLAG_NUMERICS_REFERENCE_FMA2))
        return fail(-2, "a motion pass takes the scan-mode and numerics flags only (flags 0x%x)", p->flags);
    { const int nm = p->flags & (RTW_FLAG_NUMERICS_CONTRACT | RTW_FLAG_NUMERICS_REFERENCE_FMA2);
      if (nm & (nm - 1)) return fail(-2, "the RTW_FLAG_NUMERICS_* bits exclude each other (flags 0x%x)", p->flags); }
    if (const int64_t rc = rtw_denoise_work_bytes(p->width, p->height, elem_bytes); rc < 0) return (int)rc;         // (the denoiser's frame rule)
    return 0;
}

// The motion table of a frame (include/rtw_hip.h rtw_motion_table_*): row k = c_cur - c_prev of sphere k, one subtraction in T per component,
// and 0; three quiet NaNs for a sphere the previous scene does not have or has with another radius (bitwise).
template <typename T, typename SceneT>
int motion_table(const SceneT *prev, const SceneT *cur, T *table) {
    if (!prev || !cur || !table) return fail(-1, "null argument");
    if (prev->n < 0 || cur->n < 0) return fail(-2, "negative sphere count");
    if (s_has_bad_scene(prev) || s_has_bad_scene(cur)) return fail(-1, "null scene array");
    const T nan = std::numeric_limits<T>::quiet_NaN();
    for (int k = 0; k < cur->n; ++k) {
        T *e = table + 4 * (size_t)k;
        const bool same = k < prev->n && memcmp(&prev->r[k], &cur->r[k], sizeof(T)) == 0;
        e[0] = same ? cur->cx[k] - prev->cx[k] : nan;
        e[1] = same ? cur->cy[k] - prev->cy[k] : nan;
        e[2] = same ? cur->cz[k] - prev->cz[k] : nan;
        e[3] = T(0);
    }
    return 0;
}

// Enqueue the pass on `stream` of the scene's device (validate_motion has accepted `p`): ONE launch, no record -- rtw_stats() is left alone.
template <typename T, typename CamT>
int launch_motion(rtw_scene_handle scene, const CamT *cam, const rtw_params *p, const void *d_table, void *d_motion, hipStream_t stream) {
    using V = typename rtw::DnVec<T>::type;
    rtw::MoParams<T> U;
    memset(&U, 0, sizeof U);
    for (int k = 0; k < 3; ++k) { U.o[k] = cam->origin[k]; U.llc[k] = cam->lower_left_corner[k]; U.hor[k] = cam->horizontal[k]; U.ver[k] = cam->vertical[k]; }
    U.W = p->width; U.H = p->height;
    // the caller's order (ties go by it) and the 24 KB rule of every kernel that stages the scene
    PlainView<T> S;
    if (int rc = plain_scene_view<T>(scene, false, numerics_of(p->flags), &S)) return rc;
    const long long n_pix = (long long)p->width * p->height;
    const unsigned grid = (unsigned)((n_pix + 255) / 256);
    // (measurement aid, tools/gpu_animation.py: events around the kernel, reported on stderr -- this one blocks)
    static const bool profile = aid_flag("RTW_TEMPORAL_PROFILE");
    StageMarks marks(profile, stream);
    HIP_TRY(marks.mark());
    (void)hipGetLastError();
    if (S.lds_scene) hipLaunchKernelGGL((rtw::motion_pass<T, true>), dim3(grid), dim3(256), S.scene_bytes, stream, U, S.scene, (const V *)d_table, (V *)d_motion);
    else hipLaunchKernelGGL((rtw::motion_pass<T, false>), dim3(grid), dim3(256), 0, stream, U, S.scene, (const V *)d_table, (V *)d_motion);
    HIP_TRY(hipGetLastError());
    if (profile) {
        HIP_TRY(marks.mark());
        HIP_TRY(marks.measure());
        fprintf(stderr, "[rtw motion] %s %dx%d spheres=%d lds_scene=%d ms=%.5f\n", sizeof(T) == 8 ? "f64" : "f32", p->width, p->height, scene->n, (int)S.lds_scene, marks.ms[0]);
    }
    return 0;
}

// The device-resident entry point: nulls, the parameters, the pointers' alignment, then the handle and what needs it (the table's extent).
template <typename T, typename CamT>
int motion_device(rtw_scene_handle scene, const CamT *cam, const rtw_params *p, const void *d_table, void *d_motion, void *stream_v) {
    if (!p) return fail(-1, "null params");
    if (!scene || !cam || !d_motion) return fail(-1, "null argument");
    if (int rc = validate_motion(p, (int)sizeof(T))) return rc;
    if (((uintptr_t)d_motion & 15u) || ((uintptr_t)d_table & 15u)) return fail(-2, "the motion plane and the motion table must be 16-byte aligned");
    if (scene->is_f64 != (sizeof(T) == 8)) return fail(-4, "scene handle precision does not match the call");
    if (p->device >= 0 && p->device != scene->device) return fail(-4, "params.device %d != scene device %d", p->device, scene->device);
    const size_t mo_b = (size_t)p->width * (size_t)p->height * 4 * sizeof(T), tab_b = (size_t)scene->n * 4 * sizeof(T);
    if (d_table && ranges_overlap(d_motion, mo_b, d_table, tab_b)) return fail(-2, "d_motion may not alias the table");
    DeviceGuard guard;
    HIP_TRY(hipSetDevice(scene->device));
    return launch_motion<T>(scene, cam, p, d_table, d_motion, (hipStream_t)stream_v);
}

template int motion_table<float>(const rtw_scene_f32 *, const rtw_scene_f32 *, float *);
template int motion_table<double>(const rtw_scene_f64 *, const rtw_scene_f64 *, double *);
template int launch_motion<float>(rtw_scene_handle, const rtw_camera_f32 *, const rtw_params *, const void *, void *, hipStream_t);
template int launch_motion<double>(rtw_scene_handle, const rtw_camera_f64 *, const rtw_params *, const void *, void *, hipStream_t);

}  // namespace rtwh

using namespace rtwh;

extern "C" {

int rtw_motion_table_f32(const rtw_scene_f32 *scene_prev, const rtw_scene_f32 *scene, void *table) { return motion_table<float>(scene_prev, scene, (float *)table); }
int rtw_motion_table_f64(const rtw_scene_f64 *scene_prev, const rtw_scene_f64 *scene, void *table) { return motion_table<double>(scene_prev, scene, (double *)table); }
int rtw_first_hit_motion_device_f32(rtw_scene_handle scene, const rtw_camera_f32 *cam, const rtw_params *p, const void *d_table, void *d_motion, void *hip_stream) {
    return motion_device<float>(scene, cam, p, d_table, d_motion, hip_stream);
}
int rtw_first_hit_motion_device_f64(rtw_scene_handle scene, const rtw_camera_f64 *cam, const rtw_params *p, const void *d_table, void *d_motion, void *hip_stream) {
    return motion_device<double>(scene, cam, p, d_table, d_motion, hip_stream);
}

}  // extern "C"
