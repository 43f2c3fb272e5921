/* A wide aperture from C (include/rtw_hip.h rtw_render_wide_aperture_f32): the two-sphere scene through a camera whose aperture gives the
 * far field a circle of confusion beyond the defocus stage's 8 px -- once sampled on the lens by the trace kernel (lens.ppm: noisy where
 * it is out of focus) and once rendered through the pinhole, filtered, and given its lens afterwards by the wide-aperture stage with
 * circles of up to 32 px (wide_aperture.ppm), in one call, the frame copied back once.
 *   gcc -std=c99 -Iinclude examples/render_wide_aperture_c.c -Lraytracingweekend.jl_amd/lib -lrtw_hip -Wl,-rpath,$PWD/raytracingweekend.jl_amd/lib -lm -o render_wide_aperture_c
 *   ./render_wide_aperture_c [width 400] [spp 4]
 * tests/test_wide_aperture_abi.py compiles and links it (no GPU needed for that); running it needs a GPU. */
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

int main(int argc, char **argv) {
    const int width = argc > 1 ? atoi(argv[1]) : 400, spp = argc > 2 ? atoi(argv[2]) : 4;
    const int height = width * 9 / 16;
    if (width <= 0 || height <= 0 || spp <= 0) return 2;
    const float cx[2] = {0.0f, 0.0f}, cy[2] = {0.0f, -100.5f}, cz[2] = {-1.0f, -1.0f}, r[2] = {0.5f, 100.0f};
    const int32_t kind[2] = {RTW_LAMBERTIAN, RTW_LAMBERTIAN};
    const float ar[2] = {0.7f, 0.8f}, ag[2] = {0.3f, 0.8f}, ab[2] = {0.3f, 0.0f}, param[2] = {0.0f, 0.0f};
    rtw_scene_f32 scene = {2, cx, cy, cz, r, kind, ar, ag, ab, param};
    /* default_camera((0,0,0), (0,0,-1), (0,1,0), 90, 16/9, aperture 0.1, focus 0.5) (src/camera.jl:18-36): the viewport scales with the focus */
    rtw_camera_f32 cam;
    memset(&cam, 0, sizeof cam);
    const float focus = 0.5f, vh = 2.0f * focus, vw = 16.0f / 9.0f * vh;
    cam.horizontal[0] = vw; cam.vertical[1] = vh;
    cam.lower_left_corner[0] = -vw / 2; cam.lower_left_corner[1] = -vh / 2; cam.lower_left_corner[2] = -focus;
    cam.u[0] = 1.0f; cam.v[1] = 1.0f; cam.w[2] = 1.0f;
    cam.lens_radius = 0.1f;                                   /* K = 0.1 * width / 1.78: 22 px at the default width */
    rtw_params p;
    memset(&p, 0, sizeof p);
    p.width = width; p.height = height; p.spp = spp; p.max_depth = 16; p.seed = 1;
    p.shard_count = 1; p.device = -1; p.gamma = 1;
    rtw_denoise_t d;
    memset(&d, 0, sizeof d);
    d.levels = 3; d.normal_power_log2 = 1; d.flags = RTW_DENOISE_DEMODULATE; d.gamma = 1; d.device = -1;
    d.sigma_color = 0.5; d.sigma_depth = 0.1;
    rtw_wide_aperture_t b;
    memset(&b, 0, sizeof b);
    b.max_radius = RTW_WIDE_APERTURE_MAX_RADIUS; b.gamma = 1; b.device = -1;
    b.lens_radius = -1.0;                                      /* the camera's own aperture */
    b.focus_dist = 0.0;                                        /* the camera's own focus plane */
    if (rtw_abi_version() != RTW_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 2; }
    const size_t n_pix = (size_t)width * height;
    float *lens = (float *)malloc(n_pix * 3 * sizeof(float)), *soft = (float *)malloc(n_pix * 3 * sizeof(float));
    if (!lens || !soft) return 2;

    CHECK(rtw_render_f32(&scene, &cam, &p, lens));             /* the lens sampled by the trace kernel */
    CHECK(rtw_render_wide_aperture_f32(&scene, &cam, &p, &d, &b, soft));
    rtw_stats_t st;
    CHECK(rtw_stats(&st));                                     /* the pinhole render inside the second call */
    double diff = 0;
    for (size_t k = 0; k < n_pix * 3; ++k) diff += fabs((double)soft[k] - (double)lens[k]);
    fprintf(stderr, "%d x %d at %d spp: trace kernel %.3f ms; the two frames differ by %.4f per channel on average\n", width, height, spp, st.kernel_ms,
            diff / (double)(n_pix * 3));
    if (write_ppm("lens.ppm", width, height, lens) || write_ppm("wide_aperture.ppm", width, height, soft)) return 2;
    free(lens); free(soft);
    rtw_shutdown();
    return 0;
}
