/* First-hit feature buffers from C (include/rtw_hip.h rtw_render_features_f32): albedo, normal, depth and coverage of the two-sphere
 * scene for the primary rays of a render of `spp` samples -- the guides a denoiser wants next to the image.  Writes features_normal.ppm
 * (n / coverage mapped from [-1, 1] to [0, 255]; black where nothing is hit) and features_albedo.ppm, and prints the coverage census.
 *   gcc -std=c99 -Iinclude examples/render_features_c.c -Lraytracingweekend.jl_amd/lib -lrtw_hip -Wl,-rpath,$PWD/raytracingweekend.jl_amd/lib -lm -o render_features_c
 *   ./render_features_c [width 400] [spp 16]
 * tests/test_features_abi.py compiles and links it (no GPU needed for that); running it needs a GPU. */
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
                x = x < 0 ? 0 : (x > 1 ? 1 : x);
                fputc((int)lrintf(x * 255.0f), f);
            }
    fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    const int width = argc > 1 ? atoi(argv[1]) : 400, spp = argc > 2 ? atoi(argv[2]) : 16;
    const int height = width * 9 / 16;
    if (width <= 0 || height <= 0 || spp <= 0) return 2;
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
    p.shard_count = 1; p.device = -1; p.gamma = 1;                /* n_chunks = 0: the default rule, min(spp, 256) chunks */
    if (rtw_abi_version() != RTW_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 2; }
    const int n_chunks = spp < 256 ? spp : 256;
    const int chunk_spp = (spp + n_chunks - 1) / n_chunks, n_eff = (spp + chunk_spp - 1) / chunk_spp;
    const size_t n_pix = (size_t)width * height;
    float *feat = (float *)malloc(n_pix * RTW_FEATURE_CHANNELS * sizeof(float)), *rgb = (float *)malloc(n_pix * 3 * sizeof(float));
    if (!feat || !rgb) return 2;

    CHECK(rtw_render_features_f32(&scene, &cam, &p, 0, n_eff, feat));      /* the whole render: chunks [0, N) */
    rtw_stats_t st;
    CHECK(rtw_stats(&st));
    size_t empty = 0, partial = 0;
    for (size_t k = 0; k < n_pix; ++k) {
        const float *v = feat + k * RTW_FEATURE_CHANNELS;
        const float cov = v[7];
        empty += cov == 0.0f;
        partial += cov > 0.0f && cov < 1.0f;
        for (int c = 0; c < 3; ++c) rgb[k * 3 + c] = cov > 0.0f ? 0.5f * (v[3 + c] / cov + 1.0f) : 0.0f;      /* the mean normal of the hits */
    }
    fprintf(stderr, "%d x %d, %d feature samples per pixel: %zu pixels see nothing, %zu lie on a silhouette; %llu scans in %.3f ms\n", width, height,
            n_eff, empty, partial, (unsigned long long)st.segments, st.kernel_ms);
    if (write_ppm("features_normal.ppm", width, height, rgb)) return 2;
    for (size_t k = 0; k < n_pix; ++k)
        for (int c = 0; c < 3; ++c) rgb[k * 3 + c] = feat[k * RTW_FEATURE_CHANNELS + c];      /* albedo: sky where nothing is hit */
    if (write_ppm("features_albedo.ppm", width, height, rgb)) return 2;
    free(feat); free(rgb);
    rtw_shutdown();
    return 0;
}
