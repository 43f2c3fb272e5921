// rtw_temporal.hip -- temporal reprojection (include/rtw_hip.h rtw_temporal_*): the checks that need no device, the host constants of a step,
// the one launch of its kernel (rtw_temporal.hpp), the step with moments and the noise map (rtw_history_moments_*, rtw_history_noise_device_*), the
// clamped step (rtw_clamped_step_device_*: the checks of its clamp and the launch of its own kernel, rtw_temporal_clamp.hpp) and the
// device-resident entry points, the step over a moving scene among them (rtw_animated_step_device_*: the MOTION instances, the plane of rtw_motion.hip); the batched forms of all three (rtw_reproject_*: n_paths paths in each launch, the table of their camera constants).
// (The host-buffer entry points live with the other cached-context paths: rtw_temporal_*, rtw_history_moments_* and rtw_clamped_step_* in rtw_stage_host.hip,
// rtw_render_sequence_*, rtw_render_path_* and rtw_render_paths_* in rtw_render_host.hip.)
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

// The camera constants of one path (include/rtw_hip.h rtw_reproject_table_*: 32 elements, the head of rtw::TpParams): the current camera's fields,
// the previous camera's and the projection's constants -- binary64 from the previous camera's fields, every dot product (x + y) + z, each
// rounded to T once.  cam_prev null (the first frame): elements 12..28 are 0.  The ONE copy of this arithmetic: launch_temporal's own
// constants and rtw_reproject_table_* both come from here.
template <typename T, typename CamT>
void temporal_table_entry(const CamT *cam, const CamT *cam_prev, T *e) {
    for (int k = 0; k < 32; ++k) e[k] = T(0);
    for (int k = 0; k < 3; ++k) { e[k] = cam->origin[k]; e[3 + k] = cam->lower_left_corner[k]; e[6 + k] = cam->horizontal[k]; e[9 + k] = cam->vertical[k]; }
    if (!cam_prev) return;
    double q[3], w[3], h[3], v[3];
    for (int k = 0; k < 3; ++k) {
        e[12 + k] = cam_prev->origin[k]; e[15 + k] = cam_prev->w[k]; e[18 + k] = cam_prev->horizontal[k]; e[21 + k] = cam_prev->vertical[k];
        q[k] = (double)cam_prev->lower_left_corner[k] - (double)cam_prev->origin[k];
        w[k] = cam_prev->w[k]; h[k] = cam_prev->horizontal[k]; v[k] = cam_prev->vertical[k];
    }
    auto dot = [](const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; };
    e[24] = (T)dot(q, w); e[25] = (T)dot(q, h); e[26] = (T)dot(q, v);
    e[27] = (T)(1.0 / dot(h, h)); e[28] = (T)(1.0 / dot(v, v));
}

// the path dimensions of a batched launch's grid: the path index is blockIdx.z * gridDim.y + blockIdx.y (rtw_temporal.hpp TpPaths)
static dim3 paths_grid(unsigned blocks, int32_t n_paths) {
    const unsigned np = (unsigned)n_paths;
    return dim3(blocks, np < rtw::TP_PATHS_Y ? np : rtw::TP_PATHS_Y, (np + rtw::TP_PATHS_Y - 1) / rtw::TP_PATHS_Y);
}

// Enqueue one step on `stream` of the current device (validate_temporal has accepted the call).  n_paths == 0: the step of ONE path -- cam_prev
// and d_state_prev are both null (the first frame) or both given.  n_paths >= 1 (rtw_reproject_batch_device_*): the step of that many paths in
// the SAME single launch -- cam and cam_prev are unused, the constants of path s are entry s of the device table d_table, every buffer holds
// the paths one behind the other (states and moment planes at their byte sizes), d_state_prev null: every path's first frame.
// d_moment_next non-null: the step with moments (rtw_history_moments_*), d_moment_prev null exactly when
// d_state_prev is.  `c` non-null (validate_temporal_clamp has accepted it): the clamped step -- its own kernel (rtw_temporal_clamp.hpp), one workgroup per
// tile, whenever there is a previous state; the first frame is the plain step's.
// d_motion non-null (rtw_animated_step_device_*; one path, a previous state): the MOTION instance of whichever kernel runs.
template <typename T, typename CamT>
int launch_temporal(const rtw_temporal_t *t, const CamT *cam, const CamT *cam_prev, int32_t n_paths, const void *d_table, int32_t width, int32_t height, const void *d_image,
                    const void *d_features, const void *d_state_prev, void *d_state_next, void *d_out, hipStream_t stream, const void *d_moment_prev, void *d_moment_next,
                    const rtw_temporal_clamp_t *c, const void *d_motion) {
    using V = typename rtw::DnVec<T>::type;
    if (d_motion && (n_paths || !d_state_prev)) return fail(-9, "internal: a motion plane goes with one path's step behind the first frame");
    const long long n_pix = (long long)width * height;
    rtw::TpParams<T> U;
    memset(&U, 0, sizeof U);
    static_assert(offsetof(rtw::TpParams<T>, inv_sz) == 29 * sizeof(T), "a table entry is the head of TpParams");
    if (!n_paths) {
        T e[32];
        temporal_table_entry<T>(cam, cam_prev, e);
        memcpy(&U, e, 29 * sizeof(T));
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
    rtw::TpTail<T, true, false> B;
    B.table = (const T *)d_table; B.st_stride = state_bytes(width, height, sizeof(T)); B.mo_stride = moment_bytes(width, height, sizeof(T)); B.n_paths = (unsigned)n_paths;
    rtw::TpTail<T, false, true> Q;
    Q.plane = (const V *)d_motion;
    // (measurement aid, tools/gpu_temporal.py: events around the kernel, reported on stderr -- this one blocks)
    static const bool profile = aid_flag("RTW_TEMPORAL_PROFILE");
    StageMarks marks(profile, stream);
    HIP_TRY(marks.mark());
    (void)hipGetLastError();
    const T *mp = (const T *)d_moment_prev;
    T *mn = (T *)d_moment_next;
    // the previous state's planes (the first frame: null, its instances read none) and the next state's
    const V *ep = sp ? (const V *)sp : nullptr, *gp = sp ? (const V *)(sp + pb) : nullptr;
    const T *lp = sp ? (const T *)(sp + 2 * pb) : nullptr;
    if (c && sp) {
        // the tile grid: fewer tiles than the frame rule's 8 x 8 ones, so one 32-bit grid dimension holds them
        rtw::TpClampParams<T> K;
        memset(&K, 0, sizeof K);
        K.ks = (T)c->sigma; K.ls = (T)c->len_scale; K.r = c->radius;
        K.tiles_i = (unsigned)((height + rtw::TP_TI - 1) / rtw::TP_TI);
        const unsigned tiles = K.tiles_i * (unsigned)((width + rtw::TP_TJ - 1) / rtw::TP_TJ);
        auto go = [&](auto mo, auto gd) {
            if (n_paths) hipLaunchKernelGGL((rtw::tp_step_clamped<T, decltype(mo)::value, decltype(gd)::value, true>), paths_grid(tiles, n_paths), dim3(256), 0, stream, U, K, (const T *)d_image,
                                            (const V *)d_features, ep, gp, lp, (V *)sn, (V *)(sn + pb), (T *)(sn + 2 * pb), (T *)d_out, mp, mn, B);
            else if (d_motion) hipLaunchKernelGGL((rtw::tp_step_clamped<T, decltype(mo)::value, decltype(gd)::value, false, true>), dim3(tiles), dim3(256), 0, stream, U, K, (const T *)d_image,
                                                  (const V *)d_features, ep, gp, lp, (V *)sn, (V *)(sn + pb), (T *)(sn + 2 * pb), (T *)d_out, mp, mn, Q);
            else hipLaunchKernelGGL((rtw::tp_step_clamped<T, decltype(mo)::value, decltype(gd)::value, false>), dim3(tiles), dim3(256), 0, stream, U, K, (const T *)d_image,
                                    (const V *)d_features, ep, gp, lp, (V *)sn, (V *)(sn + pb), (T *)(sn + 2 * pb), (T *)d_out, mp, mn, rtw::TpTail<T, false, false>());
        };
        const bool gd = (c->flags & RTW_CLAMP_GUIDES) != 0;
        if (mn) { if (gd) go(std::true_type(), std::true_type()); else go(std::true_type(), std::false_type()); }
        else { if (gd) go(std::false_type(), std::true_type()); else go(std::false_type(), std::false_type()); }
    } else {
        auto go = [&](auto hp, auto mo) {
            if (n_paths) hipLaunchKernelGGL((rtw::tp_step<T, decltype(hp)::value, decltype(mo)::value, true>), paths_grid(grid, n_paths), dim3(256), 0, stream, U, (const T *)d_image,
                                            (const V *)d_features, ep, gp, lp, (V *)sn, (V *)(sn + pb), (T *)(sn + 2 * pb), (T *)d_out, mp, mn, B);
            else hipLaunchKernelGGL((rtw::tp_step<T, decltype(hp)::value, decltype(mo)::value, false>), dim3(grid), dim3(256), 0, stream, U, (const T *)d_image, (const V *)d_features, ep,
                                    gp, lp, (V *)sn, (V *)(sn + pb), (T *)(sn + 2 * pb), (T *)d_out, mp, mn, rtw::TpTail<T, false, false>());
        };
        // (the plain step over a moving scene: the two HAS_PREV instances with the motion plane)
        auto gom = [&](auto mo) {
            hipLaunchKernelGGL((rtw::tp_step<T, true, decltype(mo)::value, false, true>), dim3(grid), dim3(256), 0, stream, U, (const T *)d_image, (const V *)d_features, ep, gp, lp, (V *)sn,
                               (V *)(sn + pb), (T *)(sn + 2 * pb), (T *)d_out, mp, mn, Q);
        };
        if (d_motion) { if (mn) gom(std::true_type()); else gom(std::false_type()); }
        else if (mn) { if (sp) go(std::true_type(), std::true_type()); else go(std::false_type(), std::true_type()); }
        else { if (sp) go(std::true_type(), std::false_type()); else go(std::false_type(), std::false_type()); }
    }
    HIP_TRY(hipGetLastError());
    if (profile) {
        HIP_TRY(marks.mark());
        HIP_TRY(marks.measure());
        const float ms = marks.ms[0];
        if (c && sp) fprintf(stderr, "[rtw temporal] %s %dx%d %s r=%d guides=%d paths=%d ms=%.5f\n", sizeof(T) == 8 ? "f64" : "f32", width, height, d_motion ? (mn ? "clamped+moments+motion" : "clamped+motion") : mn ? "clamped+moments" : "clamped", c->radius, c->flags & RTW_CLAMP_GUIDES, n_paths, ms);
        else fprintf(stderr, "[rtw temporal] %s %dx%d %s prev=%d paths=%d ms=%.5f\n", sizeof(T) == 8 ? "f64" : "f32", width, height, d_motion ? (mn ? "step+moments+motion" : "step+motion") : mn ? "step+moments" : "step", sp ? 1 : 0, n_paths, ms);
    }
    return 0;
}

template <typename T, typename CamT>
void temporal_table(const CamT *cams, const CamT *cams_prev, int64_t n, T *table) {
    for (int64_t s = 0; s < n; ++s) temporal_table_entry<T>(cams + s, cams_prev ? cams_prev + s : nullptr, table + 32 * s);
}

// Enqueue the noise map of a state and its moment plane on `stream` of the current device (validate_temporal_noise has accepted the call): ONE launch.
// n_paths >= 1 (rtw_reproject_noise_batch_device_*): the maps of that many states and planes, one behind the other, in the same single launch.
template <typename T>
int launch_temporal_noise(const rtw_temporal_noise_t *n, int32_t width, int32_t height, int32_t n_paths, const void *d_state, const void *d_moment, void *d_noise, hipStream_t stream) {
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
    StageMarks marks(profile, stream);
    HIP_TRY(marks.mark());
    (void)hipGetLastError();
    if (n_paths) hipLaunchKernelGGL((rtw::tp_noise<T, true>), paths_grid(grid, n_paths), dim3(256), 0, stream, U, (const V *)sp, (const V *)(sp + pb), (const T *)(sp + 2 * pb), (const T *)d_moment,
                                    (T *)d_noise, rtw::TpPaths<T, true>{nullptr, state_bytes(width, height, sizeof(T)), moment_bytes(width, height, sizeof(T)), (unsigned)n_paths});
    else hipLaunchKernelGGL((rtw::tp_noise<T, false>), dim3(grid), dim3(256), 0, stream, U, (const V *)sp, (const V *)(sp + pb), (const T *)(sp + 2 * pb), (const T *)d_moment, (T *)d_noise,
                            rtw::TpPaths<T, false>());
    HIP_TRY(hipGetLastError());
    if (profile) {
        HIP_TRY(marks.mark());
        HIP_TRY(marks.measure());
        const float ms = marks.ms[0];
        fprintf(stderr, "[rtw temporal] %s %dx%d noise r=%d paths=%d ms=%.5f\n", sizeof(T) == 8 ? "f64" : "f32", width, height, n->radius, n_paths, ms);
    }
    return 0;
}

// The device-resident entry points of a step: nulls, the parameters, then the pointers' alignment and aliasing.  `moments`:
// rtw_history_moments_device_*, the same with the two moment planes (d_moment_prev null exactly when d_state_prev is).  `clamped`:
// rtw_clamped_step_device_*, either of the two with the clamp `c`.  `animated`: rtw_animated_step_device_*, any of the three over a moving
// scene -- the motion plane d_motion is there exactly when the previous state is.
template <typename T, typename CamT>
int temporal_device(const rtw_temporal_t *t, const CamT *cam, const CamT *cam_prev, int32_t width, int32_t height, const void *d_image, const void *d_features, const void *d_state_prev,
                    void *d_state_next, void *d_out, void *stream_v, bool moments = false, const void *d_moment_prev = nullptr, void *d_moment_next = nullptr, bool clamped = false,
                    const rtw_temporal_clamp_t *c = nullptr, bool animated = false, const void *d_motion = nullptr) {
    if (!t || !cam || !d_image || !d_features || !d_state_next || !d_out || (moments && !d_moment_next) || (clamped && !c)) return fail(-1, "null argument");
    if (int rc = validate_temporal(t, width, height, (int)sizeof(T))) return rc;
    if (clamped) if (int rc = validate_temporal_clamp(c)) return rc;
    if ((cam_prev == nullptr) != (d_state_prev == nullptr)) return fail(-2, "cam_prev and d_state_prev must both be given or both be null (the first frame)");
    if (moments && (d_moment_prev == nullptr) != (d_state_prev == nullptr)) return fail(-2, "d_moment_prev and d_state_prev must both be given or both be null (the first frame)");
    if (moments && (((uintptr_t)d_moment_prev & 15u) || ((uintptr_t)d_moment_next & 15u))) return fail(-2, "both moment planes must be 16-byte aligned");
    if (animated && (d_motion == nullptr) != (d_state_prev == nullptr)) return fail(-2, "d_motion and d_state_prev must both be given or both be null (the first frame)");
    if ((uintptr_t)d_motion & 15u) return fail(-2, "the motion plane must be 16-byte aligned");
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
    if (d_motion) {
        const size_t mv_b = n_pix * 4 * sizeof(T);
        if (ranges_overlap(d_motion, mv_b, d_out, img_b) || ranges_overlap(d_motion, mv_b, d_state_next, st_b) ||
            (moments && ranges_overlap(d_motion, mv_b, d_moment_next, (size_t)moment_bytes(width, height, sizeof(T)))))
            return fail(-2, "d_motion may not alias an output");
    }
    DeviceGuard guard;
    if (t->device >= 0) HIP_TRY(hipSetDevice(t->device));
    return launch_temporal<T>(t, cam, cam_prev, 0, nullptr, width, height, d_image, d_features, d_state_prev, d_state_next, d_out, (hipStream_t)stream_v, moments ? d_moment_prev : nullptr,
                              moments ? d_moment_next : nullptr, clamped ? c : nullptr, d_motion);
}

// the batch's own size rule: the batched filter's frame rule on (width, height, number of frames)
static int check_paths_size(int32_t width, int32_t height, int32_t n_paths) {
    if ((double)width * (double)height * (double)n_paths >= (double)(1ll << 39)) return fail(-5, "batch too large for one call: %d paths of %d x %d pixels", n_paths, width, height);
    return 0;
}

// The device-resident entry point of a batched step (rtw_reproject_batch_device_*): nulls, the count, the parameters, the batch's size, then
// the pointers' pairing, alignment and aliasing over the extents of all n_paths paths.  `c` null: plain steps; both moment pointers null: no moments.
template <typename T>
int temporal_batch_device(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, int32_t n_paths, const void *d_table, int32_t width, int32_t height, const void *d_images,
                          const void *d_features, const void *d_states_prev, const void *d_moments_prev, void *d_states_next, void *d_moments_next, void *d_out, void *stream_v) {
    const bool moments = d_moments_prev || d_moments_next;
    if (!t || !d_table || !d_images || !d_features || !d_states_next || !d_out || (moments && !d_moments_next)) return fail(-1, "null argument");
    if (n_paths < 1) return fail(-2, "n_paths must be >= 1 (got %d)", n_paths);
    if (int rc = validate_temporal(t, width, height, (int)sizeof(T))) return rc;
    if (c) if (int rc = validate_temporal_clamp(c)) return rc;
    if (int rc = check_paths_size(width, height, n_paths)) return rc;
    if (moments && (d_moments_prev == nullptr) != (d_states_prev == nullptr)) return fail(-2, "d_moments_prev and d_states_prev must both be given or both be null (the first frame)");
    if (((uintptr_t)d_table & 15u) || ((uintptr_t)d_features & 15u) || ((uintptr_t)d_states_prev & 15u) || ((uintptr_t)d_states_next & 15u) || ((uintptr_t)d_moments_prev & 15u) ||
        ((uintptr_t)d_moments_next & 15u))
        return fail(-2, "the table, the feature buffer, the states and the moment planes must be 16-byte aligned");
    if (((uintptr_t)d_images & (sizeof(T) - 1)) || ((uintptr_t)d_out & (sizeof(T) - 1))) return fail(-2, "the image buffers must be aligned to their element type");
    const size_t np = (size_t)n_paths, n_pix = (size_t)width * (size_t)height * np;
    // every output against the outputs behind it and against every input that is there
    const size_t img_b = n_pix * 3 * sizeof(T), st_b = (size_t)state_bytes(width, height, sizeof(T)) * np, mo_b = (size_t)moment_bytes(width, height, sizeof(T)) * np;
    if (int rc = check_alias({{"d_out", d_out, img_b}, {"d_states_next", d_states_next, st_b}, {"d_moments_next", d_moments_next, mo_b}},
                             {{"d_images", d_images, img_b}, {"d_features", d_features, n_pix * 8 * sizeof(T)}, {"d_states_prev", d_states_prev, st_b}, {"d_moments_prev", d_moments_prev, mo_b},
                              {"d_table", d_table, np * 32 * sizeof(T)}}))
        return rc;
    DeviceGuard guard;
    if (t->device >= 0) HIP_TRY(hipSetDevice(t->device));
    using CamT = std::conditional_t<sizeof(T) == 8, rtw_camera_f64, rtw_camera_f32>;
    return launch_temporal<T, CamT>(t, nullptr, nullptr, n_paths, d_table, width, height, d_images, d_features, d_states_prev, d_states_next, d_out, (hipStream_t)stream_v,
                                              d_moments_prev, d_moments_next, c, nullptr);
}

// ... and of the batched noise map (rtw_reproject_noise_batch_device_*)
template <typename T>
int temporal_noise_batch_device(const rtw_temporal_noise_t *n, int32_t width, int32_t height, int32_t n_paths, const void *d_states, const void *d_moments, void *d_noise, void *stream_v) {
    if (!n || !d_states || !d_moments || !d_noise) return fail(-1, "null argument");
    if (n_paths < 1) return fail(-2, "n_paths must be >= 1 (got %d)", n_paths);
    if (int rc = validate_temporal_noise(n, width, height, (int)sizeof(T))) return rc;
    if (int rc = check_paths_size(width, height, n_paths)) return rc;
    if (((uintptr_t)d_states & 15u) || ((uintptr_t)d_moments & 15u)) return fail(-2, "the states and the moment planes must be 16-byte aligned");
    if ((uintptr_t)d_noise & (sizeof(T) - 1)) return fail(-2, "the noise maps must be aligned to their element type");
    const size_t np = (size_t)n_paths, noise_b = (size_t)width * (size_t)height * np * sizeof(T);
    if (int rc = check_alias({{"d_noise", d_noise, noise_b}}, {{"d_states", d_states, (size_t)state_bytes(width, height, sizeof(T)) * np}, {"d_moments", d_moments, (size_t)moment_bytes(width, height, sizeof(T)) * np}}))
        return rc;
    DeviceGuard guard;
    if (n->device >= 0) HIP_TRY(hipSetDevice(n->device));
    return launch_temporal_noise<T>(n, width, height, n_paths, d_states, d_moments, d_noise, (hipStream_t)stream_v);
}

// The device-resident entry point of the noise map: nulls, the parameters, then the pointers' alignment and aliasing.
template <typename T>
int temporal_noise_device(const rtw_temporal_noise_t *n, int32_t width, int32_t height, const void *d_state, const void *d_moment, void *d_noise, void *stream_v) {
    if (!n || !d_state || !d_moment || !d_noise) return fail(-1, "null argument");
    if (int rc = validate_temporal_noise(n, width, height, (int)sizeof(T))) return rc;
    if (((uintptr_t)d_state & 15u) || ((uintptr_t)d_moment & 15u)) return fail(-2, "the state and the moment plane must be 16-byte aligned");
    if ((uintptr_t)d_noise & (sizeof(T) - 1)) return fail(-2, "the noise map must be aligned to its element type");
    const size_t n_pix = (size_t)width * (size_t)height;
    if (int rc = check_alias({{"d_noise", d_noise, n_pix * sizeof(T)}}, {{"d_state", d_state, (size_t)state_bytes(width, height, sizeof(T))}, {"d_moment", d_moment, (size_t)moment_bytes(width, height, sizeof(T))}}))
        return rc;
    DeviceGuard guard;
    if (n->device >= 0) HIP_TRY(hipSetDevice(n->device));
    return launch_temporal_noise<T>(n, width, height, 0, d_state, d_moment, d_noise, (hipStream_t)stream_v);
}

template int launch_temporal<float>(const rtw_temporal_t *, const rtw_camera_f32 *, const rtw_camera_f32 *, int32_t, const void *, int32_t, int32_t, const void *, const void *, const void *, void *, void *, hipStream_t, const void *, void *, const rtw_temporal_clamp_t *, const void *);
template int launch_temporal<double>(const rtw_temporal_t *, const rtw_camera_f64 *, const rtw_camera_f64 *, int32_t, const void *, int32_t, int32_t, const void *, const void *, const void *, void *, void *, hipStream_t, const void *, void *, const rtw_temporal_clamp_t *, const void *);
template void temporal_table<float>(const rtw_camera_f32 *, const rtw_camera_f32 *, int64_t, float *);
template void temporal_table<double>(const rtw_camera_f64 *, const rtw_camera_f64 *, int64_t, double *);
template int launch_temporal_noise<float>(const rtw_temporal_noise_t *, int32_t, int32_t, int32_t, const void *, const void *, void *, hipStream_t);
template int launch_temporal_noise<double>(const rtw_temporal_noise_t *, int32_t, int32_t, int32_t, const void *, const void *, void *, hipStream_t);

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
int rtw_animated_step_device_f32(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width, int32_t height,
                                 const void *d_image, const void *d_features, const void *d_motion, const void *d_state_prev, void *d_state_next, const void *d_moment_prev,
                                 void *d_moment_next, void *d_out, void *hip_stream) {
    return temporal_device<float>(t, cam, cam_prev, width, height, d_image, d_features, d_state_prev, d_state_next, d_out, hip_stream, d_moment_prev || d_moment_next, d_moment_prev,
                                  d_moment_next, c != nullptr, c, true, d_motion);
}
int rtw_animated_step_device_f64(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width, int32_t height,
                                 const void *d_image, const void *d_features, const void *d_motion, const void *d_state_prev, void *d_state_next, const void *d_moment_prev,
                                 void *d_moment_next, void *d_out, void *hip_stream) {
    return temporal_device<double>(t, cam, cam_prev, width, height, d_image, d_features, d_state_prev, d_state_next, d_out, hip_stream, d_moment_prev || d_moment_next, d_moment_prev,
                                   d_moment_next, c != nullptr, c, true, d_motion);
}
int rtw_history_noise_device_f32(const rtw_temporal_noise_t *n, int32_t width, int32_t height, const void *d_state, const void *d_moment, void *d_noise, void *hip_stream) {
    return temporal_noise_device<float>(n, width, height, d_state, d_moment, d_noise, hip_stream);
}
int rtw_history_noise_device_f64(const rtw_temporal_noise_t *n, int32_t width, int32_t height, const void *d_state, const void *d_moment, void *d_noise, void *hip_stream) {
    return temporal_noise_device<double>(n, width, height, d_state, d_moment, d_noise, hip_stream);
}
int64_t rtw_reproject_table_bytes(int32_t n_paths, int32_t elem_bytes) {
    if (elem_bytes != 4 && elem_bytes != 8) return fail(-2, "elem_bytes must be 4 or 8 (got %d)", elem_bytes);
    if (n_paths < 1) return fail(-2, "n_paths must be >= 1 (got %d)", n_paths);
    return (int64_t)n_paths * 32 * elem_bytes;
}
int rtw_reproject_table_f32(const rtw_camera_f32 *cams, const rtw_camera_f32 *cams_prev, int32_t n_paths, void *table) {
    if (!cams || !table) return fail(-1, "null argument");
    if (n_paths < 1) return fail(-2, "n_paths must be >= 1 (got %d)", n_paths);
    temporal_table<float>(cams, cams_prev, n_paths, (float *)table);
    return 0;
}
int rtw_reproject_table_f64(const rtw_camera_f64 *cams, const rtw_camera_f64 *cams_prev, int32_t n_paths, void *table) {
    if (!cams || !table) return fail(-1, "null argument");
    if (n_paths < 1) return fail(-2, "n_paths must be >= 1 (got %d)", n_paths);
    temporal_table<double>(cams, cams_prev, n_paths, (double *)table);
    return 0;
}
int rtw_reproject_batch_device_f32(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, int32_t n_paths, const void *d_table, int32_t width, int32_t height, const void *d_images,
                                   const void *d_features, const void *d_states_prev, const void *d_moments_prev, void *d_states_next, void *d_moments_next, void *d_out, void *hip_stream) {
    return temporal_batch_device<float>(t, c, n_paths, d_table, width, height, d_images, d_features, d_states_prev, d_moments_prev, d_states_next, d_moments_next, d_out, hip_stream);
}
int rtw_reproject_batch_device_f64(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, int32_t n_paths, const void *d_table, int32_t width, int32_t height, const void *d_images,
                                   const void *d_features, const void *d_states_prev, const void *d_moments_prev, void *d_states_next, void *d_moments_next, void *d_out, void *hip_stream) {
    return temporal_batch_device<double>(t, c, n_paths, d_table, width, height, d_images, d_features, d_states_prev, d_moments_prev, d_states_next, d_moments_next, d_out, hip_stream);
}
int rtw_reproject_noise_batch_device_f32(const rtw_temporal_noise_t *n, int32_t width, int32_t height, int32_t n_paths, const void *d_states, const void *d_moments, void *d_noise,
                                         void *hip_stream) {
    return temporal_noise_batch_device<float>(n, width, height, n_paths, d_states, d_moments, d_noise, hip_stream);
}
int rtw_reproject_noise_batch_device_f64(const rtw_temporal_noise_t *n, int32_t width, int32_t height, int32_t n_paths, const void *d_states, const void *d_moments, void *d_noise,
                                         void *hip_stream) {
    return temporal_noise_batch_device<double>(n, width, height, n_paths, d_states, d_moments, d_noise, hip_stream);
}

}  // extern "C"
