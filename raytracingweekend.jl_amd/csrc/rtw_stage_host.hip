// rtw_stage_host.hip -- the pure stages on host buffers (rtw_denoise_* / rtw_filter_batch_*, rtw_present_*, rtw_upsample_*, the temporal
// steps, rtw_velocity_blur_*, rtw_defocus_*, rtw_wide_aperture_*, rtw_lens_batch_*): each is its null checks, the stage's validate_*, a layout of the device buffer, the alias
// check of its host buffers and ONE call of stage_one_device (rtw_host_ctx.hpp) with the stage's launch.  A leased context's scene is
// left alone and this thread's last render (rtw_stats) is not touched.  n_views == 0 is the single-frame entry point, n_views != 0 the
// batched one (rtw_host.hpp batch_views; the lens stages, all three behind lens_host: lens_batch_views).
#include "rtw_host_ctx.hpp"

namespace rtwh {

// The filter (rtw_denoise_* / rtw_filter_batch_*): two H2D, prepare + `levels` launches for any number of frames, ONE D2H.
template <typename T>
int filter_host(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views, const T *images, const T *features, T *out) {
    if (!d || !images || !features || !out) return fail(-1, "null argument");
    if (int rc = n_views ? validate_filter_batch(d, width, height, n_views) : validate_denoise(d, width, height)) return rc;
    const DenoiseRegions<T> R(width, height, n_views);
    if (int rc = check_alias({{"out", out, R.img_b}}, {{"images", images, R.img_b}, {"features", features, R.feat_b}})) return rc;
    return stage_one_device<T>(d->device, nullptr, R.total, n_views ? "the filter's inputs" : "the denoiser's inputs", {{0, images, R.img_b}, {R.off_feat, features, R.feat_b}},
                               [&](HostCtx *hc, char *base) { return R.launch(d, width, height, n_views, base, hc->stream); }, {R.off_out, out, R.img_b});
}

// The present stage (rtw_present_*): one H2D of the frame, ONE launch, ONE D2H of the bytes.
template <typename T>
int present_host(const rtw_present_t *p, int32_t width, int32_t height, const T *image, uint8_t *out) {
    if (!p || !image || !out) return fail(-1, "null argument");
    if (int rc = validate_present(p, width, height, 0)) return rc;
    const size_t n_pix = (size_t)width * (size_t)height, img_b = n_pix * 3 * sizeof(T), out_b = n_pix * (size_t)p->channels;
    DevLayout L{img_b};
    const size_t off_out = L.add(out_b);
    if (int rc = check_alias({{"out", out, out_b}}, {{"image", image, img_b}}, "the input")) return rc;
    return stage_one_device<T>(p->device, nullptr, L.total, "the frame", {{0, image, img_b}},
                               [&](HostCtx *hc, char *base) { return launch_present<T>(p, width, height, 0, base, base + off_out, hc->stream); }, {off_out, out, out_b});
}

// The upsampler (rtw_upsample_* / rtw_upsample_batch_*): three H2D, prepare + `levels` + 1 launches for any number of views, ONE D2H.
template <typename T>
int upsample_host(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, int32_t n_views, const T *images_lo, const T *features_lo,
                  const T *features_hi, T *out) {
    if (!u || !images_lo || !features_lo || !features_hi || !out) return fail(-1, "null argument");
    if (int rc = validate_upsample(u, lo_width, lo_height, width, height, n_views, (int)sizeof(T))) return rc;
    const UpsampleRegions<T> R(lo_width, lo_height, width, height, n_views);
    if (int rc = check_alias({{"out", out, R.out_b}}, {{"images_lo", images_lo, R.img_b}, {"features_lo", features_lo, R.flo_b}, {"features_hi", features_hi, R.fhi_b}})) return rc;
    return stage_one_device<T>(u->device, nullptr, R.total, "the upsampler's inputs", {{0, images_lo, R.img_b}, {R.off_flo, features_lo, R.flo_b}, {R.off_fhi, features_hi, R.fhi_b}},
                               [&](HostCtx *hc, char *base) { return R.launch(u, lo_width, lo_height, width, height, n_views, base, hc->stream); }, {R.off_out, out, R.out_b});
}

// One temporal step (rtw_temporal_*, rtw_history_moments_*, rtw_clamped_step_*): two to four H2D, the step's launch (`c`: a clamped step)
// and, with `n`, the launch of the noise map of what it leaves, then two to four D2H (the next state, its moments, the map; the image
// last).  The moment planes take part when either is given; moment_next must then be.  `form_args`: what the entry point requires beyond
// that (n, moment_next and noise; or c) is there.  `animated` (rtw_animated_step_*): the step over a moving scene -- `motion`, the plane
// of rtw_first_hit_motion_* (width*height slots of 4 elements), is there exactly when the previous state is and goes up behind the other inputs.
template <typename T, typename CamT>
int temporal_step_host(bool form_args, const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, const rtw_temporal_noise_t *n, const CamT *cam, const CamT *cam_prev, int32_t width,
                       int32_t height, const T *image, const T *features, const void *state_prev, const void *moment_prev, void *state_next, void *moment_next, T *out, T *noise,
                       bool animated = false, const T *motion = nullptr) {
    const bool moments = moment_prev || moment_next;
    if (!form_args || !t || !cam || !image || !features || !state_next || !out || (moments && !moment_next)) return fail(-1, "null argument");
    if (int rc = validate_temporal(t, width, height, (int)sizeof(T))) return rc;
    if (n) if (int rc = validate_temporal_noise(n, width, height, (int)sizeof(T))) return rc;
    if (c) if (int rc = validate_temporal_clamp(c)) return rc;
    if ((cam_prev == nullptr) != (state_prev == nullptr)) return fail(-2, "cam_prev and state_prev must both be given or both be null (the first frame)");
    if (moments && (moment_prev == nullptr) != (state_prev == nullptr)) return fail(-2, "moment_prev and state_prev must both be given or both be null (the first frame)");
    if (animated && (motion == nullptr) != (state_prev == nullptr)) return fail(-2, "motion and state_prev must both be given or both be null (the first frame)");
    const MomentRegions<T> R(width, height, 1, false);
    DevLayout L{R.total_m};                                    // (the motion plane: behind every other region)
    const size_t motion_b = (size_t)width * (size_t)height * 4 * sizeof(T), off_motion = L.add(motion_b);
    // the outputs that are there against each other and against every input that is
    if (int rc = check_alias({{"out", out, R.img_b}, {"state_next", state_next, R.st_b}, {"moment_next", moment_next, R.mo_b}, {"noise", noise, R.noise_b}},
                             {{"image", image, R.img_b}, {"features", features, R.feat_b}, {"state_prev", state_prev, R.st_b}, {"moment_prev", moment_prev, R.mo_b}, {"motion", motion, motion_b}}))
        return rc;
    return stage_one_device<T>(t->device, nullptr, motion ? L.total : R.total_m, "the temporal step's inputs",
        {{0, image, R.img_b}, {R.off_feat, features, R.feat_b}, {R.off_st[0], state_prev, R.st_b}, {R.off_mo[0], moment_prev, R.mo_b}, {off_motion, motion, motion_b}},
        [&](HostCtx *hc, char *base) {
            int rc = launch_temporal<T>(t, cam, cam_prev, 0, nullptr, width, height, base, base + R.off_feat, state_prev ? base + R.off_st[0] : nullptr, base + R.off_st[1], base + R.off_acc,
                                        hc->stream, moment_prev ? base + R.off_mo[0] : nullptr, moments ? base + R.off_mo[1] : nullptr, c, motion ? base + off_motion : nullptr);
            if (!rc && n) rc = launch_temporal_noise<T>(n, width, height, 0, base + R.off_st[1], base + R.off_mo[1], base + R.off_noise, hc->stream);
            return rc;
        },
        {R.off_acc, out, R.img_b}, {{R.off_st[1], state_next, R.st_b}, {R.off_mo[1], moment_next, R.mo_b}, {R.off_noise, n ? noise : nullptr, R.noise_b}},
        "the next state, its moments or the noise map");
}

// The motion-blur stage (rtw_velocity_blur_*): three H2D (the image, the features, the motion plane), the stage's three launches, ONE D2H.
// The device buffer holds the three inputs, the output and the workspace.
template <typename T, typename CamT>
int motion_blur_host(const rtw_velocity_blur_t *b, const CamT *cam, const CamT *cam_prev, int32_t width, int32_t height, const T *image, const T *features, const T *motion, T *out) {
    if (!b || !cam || !cam_prev || !image || !features || !motion || !out) return fail(-1, "null argument");
    if (int rc = validate_motion_blur(b, width, height, (int)sizeof(T))) return rc;
    const size_t n_pix = (size_t)width * (size_t)height;
    const size_t img_b = n_pix * 3 * sizeof(T), feat_b = n_pix * RTW_FEATURE_CHANNELS * sizeof(T), mo_b = n_pix * 4 * sizeof(T);
    DevLayout L{img_b};
    const size_t off_feat = L.add(feat_b), off_mo = L.add(mo_b), off_out = L.add(img_b), off_work = L.add((size_t)rtw_velocity_blur_work_bytes(width, height, (int32_t)sizeof(T)));
    if (int rc = check_alias({{"out", out, img_b}}, {{"image", image, img_b}, {"features", features, feat_b}, {"motion", motion, mo_b}})) return rc;
    return stage_one_device<T>(b->device, nullptr, L.total, "the motion blur's inputs", {{0, image, img_b}, {off_feat, features, feat_b}, {off_mo, motion, mo_b}},
        [&](HostCtx *hc, char *base) { return launch_motion_blur<T>(b, cam, cam_prev, width, height, base, base + off_feat, base + off_mo, base + off_work, base + off_out, hc->stream); },
        {off_out, out, img_b});
}

// The lens stages (rtw_defocus_*, rtw_wide_aperture_*: n_views == 0, one view with max_radius in 1..top; rtw_lens_batch_*: n_views views
// of n_frames -- n_views or 1 -- input frames, top 32).  Two H2D (the images, the features) and, for a batch alone, a third (the lens table,
// built here), the stage's six launches (two when max_radius <= 8) for any number of views, ONE D2H of all outputs.  The device buffer:
// rtw_layout.hpp LensBatchLayout -- the inputs, the outputs, the workspaces and, for a batch alone, the table.  `what`: the inputs' words.
template <typename T, typename CamT>
int lens_host(int top, const char *what, const rtw_wide_aperture_t *b, const CamT *cams, int32_t n_views, int32_t n_frames, const double *lens_radii, const double *focus_dists,
              int32_t width, int32_t height, const T *images, const T *features, T *out) {
    if (!b || !cams || !images || !features || !out) return fail(-1, "null argument");
    if (n_views) if (int rc = validate_lens_batch_frame(b, n_views, n_frames, width, height, (int)sizeof(T))) return rc;
    std::vector<rtw_defocus_t> lens;
    if (int rc = validate_lens_batch(b, cams, n_views ? n_views : 1, width, height, lens_radii, focus_dists, false, top, &lens)) return rc;
    const LensBatchLayout R(sizeof(T), width, height, b->max_radius, n_views, n_frames);
    if (int rc = check_alias({{"out", out, R.out_b}}, {{n_views ? "images" : "image", images, R.img_b}, {"features", features, R.feat_b}})) return rc;
    std::vector<T> table;                                      // (a batch's alone: R.tab_b == 0 for one view, and nothing goes up)
    if (n_views) { table.resize((size_t)n_views * 32); lens_table<T>(lens, cams, width, table.data()); }
    return stage_one_device<T>(b->device, nullptr, R.total, what, {{0, images, R.img_b}, {R.off_feat, features, R.feat_b}, {R.off_tab, table.data(), R.tab_b}},
        [&](HostCtx *hc, char *base) {
            const LensViews vb = lens_views(R, n_views, base + R.off_tab);
            return launch_wide_aperture<T>(b, cams, width, height, base, base + R.off_feat, base + R.off_work, base + R.off_out, hc->stream, n_views ? &vb : nullptr);
        },
        {R.off_out, out, R.out_b});
}

}  // namespace rtwh

using namespace rtwh;

extern "C" {

int rtw_denoise_f32(const rtw_denoise_t *d, int32_t width, int32_t height, const float *image, const float *features, float *out) {
    return filter_host<float>(d, width, height, 0, image, features, out);
}
int rtw_denoise_f64(const rtw_denoise_t *d, int32_t width, int32_t height, const double *image, const double *features, double *out) {
    return filter_host<double>(d, width, height, 0, image, features, out);
}
int rtw_filter_batch_f32(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views, const float *images, const float *features, float *out) {
    return filter_host<float>(d, width, height, batch_views(n_views), images, features, out);
}
int rtw_filter_batch_f64(const rtw_denoise_t *d, int32_t width, int32_t height, int32_t n_views, const double *images, const double *features, double *out) {
    return filter_host<double>(d, width, height, batch_views(n_views), images, features, out);
}

int rtw_present_f32(const rtw_present_t *p, int32_t width, int32_t height, const float *image, uint8_t *out) { return present_host<float>(p, width, height, image, out); }
int rtw_present_f64(const rtw_present_t *p, int32_t width, int32_t height, const double *image, uint8_t *out) { return present_host<double>(p, width, height, image, out); }

int rtw_upsample_f32(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, const float *image_lo, const float *features_lo,
                     const float *features_hi, float *out) {
    return upsample_host<float>(u, lo_width, lo_height, width, height, 0, image_lo, features_lo, features_hi, out);
}
int rtw_upsample_f64(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, const double *image_lo, const double *features_lo,
                     const double *features_hi, double *out) {
    return upsample_host<double>(u, lo_width, lo_height, width, height, 0, image_lo, features_lo, features_hi, out);
}
int rtw_upsample_batch_f32(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, int32_t n_views, const float *images_lo,
                           const float *features_lo, const float *features_hi, float *out) {
    return upsample_host<float>(u, lo_width, lo_height, width, height, batch_views(n_views), images_lo, features_lo, features_hi, out);
}
int rtw_upsample_batch_f64(const rtw_upsample_t *u, int32_t lo_width, int32_t lo_height, int32_t width, int32_t height, int32_t n_views, const double *images_lo,
                           const double *features_lo, const double *features_hi, double *out) {
    return upsample_host<double>(u, lo_width, lo_height, width, height, batch_views(n_views), images_lo, features_lo, features_hi, out);
}

int rtw_temporal_f32(const rtw_temporal_t *t, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width, int32_t height, const float *image, const float *features,
                     const void *state_prev, void *state_next, float *out) {
    return temporal_step_host<float>(true, t, nullptr, nullptr, cam, cam_prev, width, height, image, features, state_prev, nullptr, state_next, nullptr, out, nullptr);
}
int rtw_temporal_f64(const rtw_temporal_t *t, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width, int32_t height, const double *image, const double *features,
                     const void *state_prev, void *state_next, double *out) {
    return temporal_step_host<double>(true, t, nullptr, nullptr, cam, cam_prev, width, height, image, features, state_prev, nullptr, state_next, nullptr, out, nullptr);
}
int rtw_history_moments_f32(const rtw_temporal_t *t, const rtw_temporal_noise_t *n, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width, int32_t height,
                             const float *image, const float *features, const void *state_prev, const void *moment_prev, void *state_next, void *moment_next, float *out, float *noise) {
    return temporal_step_host<float>(n && moment_next && noise, t, nullptr, n, cam, cam_prev, width, height, image, features, state_prev, moment_prev, state_next, moment_next, out, noise);
}
int rtw_history_moments_f64(const rtw_temporal_t *t, const rtw_temporal_noise_t *n, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width, int32_t height,
                             const double *image, const double *features, const void *state_prev, const void *moment_prev, void *state_next, void *moment_next, double *out, double *noise) {
    return temporal_step_host<double>(n && moment_next && noise, t, nullptr, n, cam, cam_prev, width, height, image, features, state_prev, moment_prev, state_next, moment_next, out, noise);
}
int rtw_clamped_step_f32(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width, int32_t height,
                             const float *image, const float *features, const void *state_prev, const void *moment_prev, void *state_next, void *moment_next, float *out) {
    return temporal_step_host<float>(c != nullptr, t, c, nullptr, cam, cam_prev, width, height, image, features, state_prev, moment_prev, state_next, moment_next, out, nullptr);
}
int rtw_clamped_step_f64(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width, int32_t height,
                             const double *image, const double *features, const void *state_prev, const void *moment_prev, void *state_next, void *moment_next, double *out) {
    return temporal_step_host<double>(c != nullptr, t, c, nullptr, cam, cam_prev, width, height, image, features, state_prev, moment_prev, state_next, moment_next, out, nullptr);
}
int rtw_animated_step_f32(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width, int32_t height,
                          const float *image, const float *features, const float *motion, const void *state_prev, void *state_next, const void *moment_prev, void *moment_next, float *out) {
    return temporal_step_host<float>(true, t, c, nullptr, cam, cam_prev, width, height, image, features, state_prev, moment_prev, state_next, moment_next, out, nullptr, true, motion);
}
int rtw_animated_step_f64(const rtw_temporal_t *t, const rtw_temporal_clamp_t *c, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width, int32_t height,
                          const double *image, const double *features, const double *motion, const void *state_prev, void *state_next, const void *moment_prev, void *moment_next, double *out) {
    return temporal_step_host<double>(true, t, c, nullptr, cam, cam_prev, width, height, image, features, state_prev, moment_prev, state_next, moment_next, out, nullptr, true, motion);
}

int rtw_velocity_blur_f32(const rtw_velocity_blur_t *b, const rtw_camera_f32 *cam, const rtw_camera_f32 *cam_prev, int32_t width, int32_t height, const float *image, const float *features,
                        const float *motion, float *out) {
    return motion_blur_host<float>(b, cam, cam_prev, width, height, image, features, motion, out);
}
int rtw_velocity_blur_f64(const rtw_velocity_blur_t *b, const rtw_camera_f64 *cam, const rtw_camera_f64 *cam_prev, int32_t width, int32_t height, const double *image, const double *features,
                        const double *motion, double *out) {
    return motion_blur_host<double>(b, cam, cam_prev, width, height, image, features, motion, out);
}
int rtw_defocus_f32(const rtw_defocus_t *b, const rtw_camera_f32 *cam, int32_t width, int32_t height, const float *image, const float *features, float *out) {
    return lens_host<float>(RTW_DEFOCUS_MAX_RADIUS, "the defocus stage's inputs", AsWideAperture(b).ptr, cam, 0, 0, nullptr, nullptr, width, height, image, features, out);
}
int rtw_defocus_f64(const rtw_defocus_t *b, const rtw_camera_f64 *cam, int32_t width, int32_t height, const double *image, const double *features, double *out) {
    return lens_host<double>(RTW_DEFOCUS_MAX_RADIUS, "the defocus stage's inputs", AsWideAperture(b).ptr, cam, 0, 0, nullptr, nullptr, width, height, image, features, out);
}
int rtw_wide_aperture_f32(const rtw_wide_aperture_t *b, const rtw_camera_f32 *cam, int32_t width, int32_t height, const float *image, const float *features, float *out) {
    return lens_host<float>(RTW_WIDE_APERTURE_MAX_RADIUS, "the wide-aperture stage's inputs", b, cam, 0, 0, nullptr, nullptr, width, height, image, features, out);
}
int rtw_wide_aperture_f64(const rtw_wide_aperture_t *b, const rtw_camera_f64 *cam, int32_t width, int32_t height, const double *image, const double *features, double *out) {
    return lens_host<double>(RTW_WIDE_APERTURE_MAX_RADIUS, "the wide-aperture stage's inputs", b, cam, 0, 0, nullptr, nullptr, width, height, image, features, out);
}
int rtw_lens_batch_f32(const rtw_wide_aperture_t *b, const rtw_camera_f32 *cams, int32_t n_views, int32_t n_frames, const double *lens_radii, const double *focus_dists,
                                int32_t width, int32_t height, const float *images, const float *features, float *out) {
    return lens_host<float>(RTW_WIDE_APERTURE_MAX_RADIUS, "the batched wide-aperture stage's inputs", b, cams, lens_batch_views(n_views), n_frames, lens_radii, focus_dists, width, height, images, features, out);
}
int rtw_lens_batch_f64(const rtw_wide_aperture_t *b, const rtw_camera_f64 *cams, int32_t n_views, int32_t n_frames, const double *lens_radii, const double *focus_dists,
                                int32_t width, int32_t height, const double *images, const double *features, double *out) {
    return lens_host<double>(RTW_WIDE_APERTURE_MAX_RADIUS, "the batched wide-aperture stage's inputs", b, cams, lens_batch_views(n_views), n_frames, lens_radii, focus_dists, width, height, images, features, out);
}

}  // extern "C"
