/* A full-size frame from a half-width render, from C (include/rtw_hip.h rtw_render_upsampled_f32): the two-sphere scene path-traced at
 * half the width (a quarter of the samples) and brought to full size under the guides of a full-size feature pass (upsampled.ppm) --
 * small render, both feature passes and the upsampler in one call, the frame copied back once.
 *   gcc -std=c99 -Iinclude examples/render_upsampled_c.c -Lraytracingweekend.jl_amd/lib -lrtw_hip -Wl,-rpath,$PWD/raytracingweekend.jl_amd/lib -lm -o render_upsampled_c
 *   ./render_upsampled_c [width 400] [spp 4]
 * tests/test_upsample_abi.py compiles and links it (no GPU needed for that); running it needs a GPU. */
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
    const int lo_width = (width + 1) / 2, lo_height = lo_width * 9 / 16;
    if (width <= 0 || height <= 0 || lo_height <= 0 || spp <= 0) return 2;
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
    rtw_params p;                                              /* the FULL frame; the call renders it at lo_width x lo_height */
    memset(&p, 0, sizeof p);
    p.width = width; p.height = height; p.spp = spp; p.max_depth = 16; p.seed = 1;
    p.shard_count = 1; p.device = -1; p.gamma = 1;
    rtw_upsample_t u;                                          /* (untuned defaults: those of the Python layer) */
    memset(&u, 0, sizeof u);
    u.levels = 2; u.normal_power_log2 = 1; u.flags = RTW_UPSAMPLE_DEMODULATE; u.gamma = 1; u.device = -1; u.hi_chunks = 0;
    u.sigma_color = 0.5; u.sigma_depth = 0.1; u.sigma_albedo = 0.2;
    if (rtw_abi_version() != RTW_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 2; }
    const size_t n_pix = (size_t)width * height;
    float *up = (float *)malloc(n_pix * 3 * sizeof(float));
    if (!up) return 2;

    CHECK(rtw_render_upsampled_f32(&scene, &cam, &p, lo_width, lo_height, &u, up));
    rtw_stats_t st;
    CHECK(rtw_stats(&st));                                     /* the small render inside the call */
    fprintf(stderr, "%d x %d from %d x %d at %d spp: trace kernel %.3f ms for %llu samples\n", width, height, lo_width, lo_height, spp, st.kernel_ms,
            (unsigned long long)st.samples);
    if (write_ppm("upsampled.ppm", width, height, up)) return 2;
    free(up);
    rtw_shutdown();
    return 0;
}
