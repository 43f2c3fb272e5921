/* An adaptive render, denoised, from C (include/rtw_hip.h rtw_accum_filtered_f32): the two-sphere scene rendered until every 8x8 tile
 * passes the stopping rule at `tolerance` or holds all `spp` samples; then ONE call resolves the accumulator, takes the first-hit features
 * of exactly the chunks each tile holds, makes the per-pixel noise map from the accumulator's half differences and runs the noise-guided
 * filter.  Prints where the tiles stopped and how far the plain and the guided result are from the unfiltered image.  Writes
 * adaptive_denoised.ppm.
 *   gcc -std=c99 -Iinclude examples/render_adaptive_denoised_c.c -Lraytracingweekend.jl_amd/lib -lrtw_hip -Wl,-rpath,$PWD/raytracingweekend.jl_amd/lib -lm -o render_adaptive_denoised_c
 *   ./render_adaptive_denoised_c [width 400] [spp 64] [tolerance 0.05]
 * tests/test_accum_denoise_abi.py compiles and links it (no GPU needed for that); running it needs a GPU. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rtw_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s: %d: %s\n", #call, rc_, rtw_last_error()); return 1; } } while (0)

static double mean_abs_diff(const float *a, const float *b, size_t n) {
    double s = 0;
    for (size_t k = 0; k < n; ++k) s += fabs((double)a[k] - (double)b[k]);
    return s / (double)n;
}

int main(int argc, char **argv) {
    const int width = argc > 1 ? atoi(argv[1]) : 400, spp = argc > 2 ? atoi(argv[2]) : 64;
    const double tolerance = argc > 3 ? atof(argv[3]) : 0.05;
    const int height = width * 9 / 16;
    if (width <= 0 || height <= 0 || spp <= 0 || !(tolerance > 0)) return 2;
    const float cx[2] = {0.0f, 0.0f}, cy[2] = {0.0f, -100.5f}, cz[2] = {-1.0f, -1.0f}, r[2] = {0.5f, 100.0f};
    const int32_t kind[2] = {RTW_LAMBERTIAN, RTW_LAMBERTIAN};
    const float ar[2] = {0.7f, 0.8f}, ag[2] = {0.3f, 0.8f}, ab[2] = {0.3f, 0.0f}, param[2] = {0.0f, 0.0f};
    rtw_scene_f32 scene = {2, cx, cy, cz, r, kind, ar, ag, ab, param};
    /* default_camera((0,0,0), (0,0,-1), (0,1,0), 90, 16/9, 0, 1) (src/camera.jl:18-36) */
    rtw_camera_f32 cam;
    memset(&cam, 0, sizeof cam);
    const float vh = 2.0f, vw = 16.0f / 9.0f * vh;
    cam.horizontal[0] = vw; cam.vertical[1] = vh;
    cam.lower_left_corner[0] = -vw / 2; cam.lower_left_corner[1] = -vh / 2; cam.lower_left_corner[2] = -1.0f;
    cam.u[0] = 1.0f; cam.v[1] = 1.0f; cam.w[2] = 1.0f;
    rtw_params p;
    memset(&p, 0, sizeof p);
    p.width = width; p.height = height; p.spp = spp; p.max_depth = 16; p.seed = 1;
    p.shard_count = 1; p.device = -1; p.gamma = 1;
    if (rtw_abi_version() != RTW_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 2; }
    rtw_adaptive_t ad;
    memset(&ad, 0, sizeof ad);                                  /* min_chunks = check_chunks = 0: the defaults */
    ad.tolerance = tolerance; ad.dark_floor = 0.03;
    rtw_denoise_t d;
    memset(&d, 0, sizeof d);
    d.levels = 3; d.normal_power_log2 = 1; d.flags = RTW_DENOISE_DEMODULATE; d.device = -1;
    d.sigma_depth = 0.1;                                        /* d.gamma is replaced by p.gamma */
    const size_t n = (size_t)width * height * 3;
    float *raw = (float *)malloc(n * sizeof(float)), *plain = (float *)malloc(n * sizeof(float)), *guided = (float *)malloc(n * sizeof(float));
    if (!raw || !plain || !guided) return 2;

    rtw_scene_handle sc;
    rtw_accum_handle acc;
    CHECK(rtw_scene_upload_f32(&scene, -1, &sc));
    CHECK(rtw_accum_create(-1, width, height, &acc));
    CHECK(rtw_render_adaptive_f32(sc, &cam, &p, &ad, acc, NULL, NULL));
    rtw_adaptive_info_t info;
    CHECK(rtw_accum_adaptive_info(acc, &info));
    fprintf(stderr, "tolerance %g: %d of %d tiles stopped by the rule, chunks per tile %d .. %d; %.1f %% of %d spp\n", info.tolerance, info.tiles_converged,
            info.n_tiles, info.min_chunks_held, info.max_chunks_held, 100.0 * (double)info.samples / ((double)width * height * spp), spp);
    CHECK(rtw_accum_resolve_host_f32(acc, 1, raw));
    d.sigma_color = 0.5;                                        /* colour units */
    CHECK(rtw_accum_filtered_f32(sc, &cam, &p, &d, acc, 0, plain));
    d.sigma_color = 1.0;                                        /* estimated standard deviations of each pixel */
    CHECK(rtw_accum_filtered_f32(sc, &cam, &p, &d, acc, 1, guided));
    rtw_stats_t st;
    CHECK(rtw_stats(&st));
    fprintf(stderr, "feature pass over what the tiles hold: %llu primary rays, %.3f ms\n", (unsigned long long)st.samples, st.kernel_ms);
    fprintf(stderr, "mean |filtered - unfiltered|: plain %.5f, noise-guided %.5f\n", mean_abs_diff(plain, raw, n), mean_abs_diff(guided, raw, n));
    CHECK(rtw_accum_free(acc));
    CHECK(rtw_scene_free(sc));
    FILE *f = fopen("adaptive_denoised.ppm", "wb");
    if (!f) return 2;
    fprintf(f, "P6\n%d %d\n255\n", width, height);
    for (int i = 0; i < height; ++i)
        for (int j = 0; j < width; ++j)
            for (int c = 0; c < 3; ++c) {
                float x = guided[((size_t)j * height + i) * 3 + c];
                x = x < 0 ? 0 : (x > 1 ? 1 : x);
                fputc((int)lrintf(x * 255.0f), f);
            }
    fclose(f);
    free(raw); free(plain); free(guided);
    rtw_shutdown();
    return 0;
}
