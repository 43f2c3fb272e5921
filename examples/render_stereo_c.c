/* A STEREO PAIR along an orbit with history reuse from C (include/rtw_hip.h rtw_render_paths_f32): a left and a right eye, 6.5 cm apart in a
 * scene whose unit is the metre, on an arc around the two-sphere scene -- two independent camera paths over one scene.  One call: ONE batched
 * render of 2*steps views, ONE batched feature pass, `steps` batched temporal steps (each launch advances BOTH eyes; an eye reuses what its own
 * previous frame accumulated, never the other eye's) with clamped history, one batched noise launch behind each step and ONE noise-guided
 * batched filter pass, the frames copied back once.  The layout is step-major: eye s at step k is cams[2*k + s] and frame 2*k + s of `out`.
 * Frame (k, s) is written to stereo_<k>_<L|R>.ppm.  With a fourth argument 0 the call runs plain steps without noise maps and without a filter
 * (c = n = d = NULL).
 *   gcc -std=c99 -Iinclude examples/render_stereo_c.c -Lraytracingweekend.jl_amd/lib -lrtw_hip -Wl,-rpath,$PWD/raytracingweekend.jl_amd/lib -lm -o render_stereo_c
 *   ./render_stereo_c [width 96] [spp 1] [steps 8] [filter 1]
 * tests/test_paths_abi.py compiles and links it (no GPU needed for that); running it needs a GPU. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rtw_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s: %d: %s\n", #call, rc_, rtw_last_error()); return 1; } } while (0)

static int write_ppm(const char *name, int width, int height, const float *rgb /* [j][i][3], in [0, 1] */) {
    FILE *f = fopen(name, "wb");
    if (!f) return 2;
    fprintf(f, "P6\n%d %d\n255\n", width, height);
    for (int i = 0; i < height; ++i)
        for (int j = 0; j < width; ++j)
            for (int c = 0; c < 3; ++c) {
                float x = rgb[((size_t)j * height + i) * 3 + c];
                x = x < 0 ? 0 : (x > 1 ? 1 : x);               /* (a NaN pixel -- not valid -- comes out white) */
                fputc((int)lrintf(x * 255.0f), f);
            }
    fclose(f);
    return 0;
}

/* a pinhole camera at `from` looking at `at`, up = +y, vertical field of view 90 degrees, aspect 16:9, focus distance 1 */
static void look_at(rtw_camera_f32 *cam, const float from[3], const float at[3]) {
    const float vh = 2.0f, vw = 16.0f / 9.0f * vh;
    float w[3], u[3], v[3], len;
    memset(cam, 0, sizeof *cam);
    for (int k = 0; k < 3; ++k) w[k] = from[k] - at[k];
    len = sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    for (int k = 0; k < 3; ++k) w[k] /= len;
    u[0] = w[2]; u[1] = 0.0f; u[2] = -w[0];                     /* cross((0, 1, 0), w) */
    len = sqrtf(u[0] * u[0] + u[2] * u[2]);
    for (int k = 0; k < 3; ++k) u[k] /= len;
    v[0] = w[1] * u[2] - w[2] * u[1]; v[1] = w[2] * u[0] - w[0] * u[2]; v[2] = w[0] * u[1] - w[1] * u[0];
    for (int k = 0; k < 3; ++k) {
        cam->origin[k] = from[k];
        cam->horizontal[k] = vw * u[k]; cam->vertical[k] = vh * v[k];
        cam->lower_left_corner[k] = from[k] - cam->horizontal[k] / 2 - cam->vertical[k] / 2 - w[k];
        cam->u[k] = u[k]; cam->v[k] = v[k]; cam->w[k] = w[k];
    }
}

int main(int argc, char **argv) {
    const int width = argc > 1 ? atoi(argv[1]) : 96, spp = argc > 2 ? atoi(argv[2]) : 1, steps = argc > 3 ? atoi(argv[3]) : 8;
    const int filter = argc > 4 ? atoi(argv[4]) : 1;
    const int height = width * 9 / 16, eyes = 2;
    if (width <= 0 || height <= 0 || spp <= 0 || steps <= 0 || steps > 4096) return 2;
    const float cx[2] = {0.0f, 0.0f}, cy[2] = {0.0f, -100.5f}, cz[2] = {-1.0f, -1.0f}, r[2] = {0.5f, 100.0f};
    const int32_t kind[2] = {RTW_LAMBERTIAN, RTW_LAMBERTIAN};
    const float ar[2] = {0.7f, 0.8f}, ag[2] = {0.3f, 0.8f}, ab[2] = {0.3f, 0.0f}, param[2] = {0.0f, 0.0f};
    rtw_scene_f32 scene = {2, cx, cy, cz, r, kind, ar, ag, ab, param};
    rtw_params p;
    memset(&p, 0, sizeof p);
    p.width = width; p.height = height; p.spp = spp; p.max_depth = 16; p.seed = 1;
    p.shard_count = 1; p.device = -1; p.gamma = 1;
    rtw_temporal_t t;
    memset(&t, 0, sizeof t);
    t.normal_power_log2 = 1; t.flags = RTW_TEMPORAL_DEMODULATE; t.gamma = 1; t.device = -1;
    t.sigma_depth = 0.1; t.min_weight = 0.25; t.history_max = 16.0;
    rtw_temporal_clamp_t c;                                    /* (the defaults: untuned) */
    memset(&c, 0, sizeof c);
    c.radius = 1; c.flags = 0; c.sigma = 1.0; c.len_scale = 1.0;
    rtw_temporal_noise_t n;                                    /* (the defaults: untuned) */
    memset(&n, 0, sizeof n);
    n.radius = 2; n.normal_power_log2 = 1; n.device = -1; n.sigma_depth = 0.1; n.min_len = 4.0;
    rtw_denoise_t d;
    memset(&d, 0, sizeof d);
    d.levels = 3; d.normal_power_log2 = 1; d.flags = RTW_DENOISE_DEMODULATE; d.gamma = 1; d.device = -1;
    d.sigma_color = 1.0; d.sigma_depth = 0.1;        /* (guided: sigma_color counts estimated standard deviations; DEMODULATE as in t) */
    if (rtw_abi_version() != RTW_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 2; }
    const size_t n_pix = (size_t)width * height, frames = (size_t)steps * eyes;
    rtw_camera_f32 *cams = (rtw_camera_f32 *)malloc(frames * sizeof *cams);
    uint64_t *seeds = (uint64_t *)malloc(frames * sizeof *seeds);
    float *out = (float *)malloc(frames * n_pix * 3 * sizeof(float));
    if (!cams || !seeds || !out) return 2;
    const float at[3] = {0.0f, 0.0f, -1.0f}, half_eye = 0.0325f;
    for (int k = 0; k < steps; ++k) {                           /* two degrees of arc per step; the eyes sit on the arc's tangent */
        const float phi = 0.0349066f * (float)k;
        for (int s = 0; s < eyes; ++s) {
            const float side = s ? half_eye : -half_eye;
            const float from[3] = {at[0] + 1.5f * sinf(phi) + side * cosf(phi), 0.4f, at[2] + 1.5f * cosf(phi) - side * sinf(phi)};
            look_at(&cams[(size_t)k * eyes + s], from, at);     /* step-major: eye s at step k */
            seeds[(size_t)k * eyes + s] = 1 + (uint64_t)k * eyes + (uint64_t)s;
        }
    }

    CHECK(rtw_render_paths_f32(&scene, cams, eyes, steps, seeds, &p, &t, filter ? &c : NULL, filter ? &n : NULL, filter ? &d : NULL, out));
    rtw_stats_t st;
    CHECK(rtw_stats(&st));                                     /* the batched render inside the call */
    fprintf(stderr, "%d eyes x %d steps of %d x %d at %d spp: trace kernel %.3f ms for %llu samples, a table of %lld bytes per step\n", eyes, steps, width, height, spp,
            st.kernel_ms, (unsigned long long)st.samples, (long long)rtw_reproject_table_bytes(eyes, 4));
    for (int k = 0; k < steps; ++k)
        for (int s = 0; s < eyes; ++s) {
            char name[64];
            snprintf(name, sizeof name, "stereo_%03d_%c.ppm", k, s ? 'R' : 'L');
            if (write_ppm(name, width, height, out + ((size_t)k * eyes + s) * n_pix * 3)) return 2;
        }
    free(cams); free(seeds); free(out);
    rtw_shutdown();
    return 0;
}
