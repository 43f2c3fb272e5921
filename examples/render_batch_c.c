/* Batched render from C (include/rtw_hip.h rtw_render_batch_f32): a turntable of the two-sphere scene -- N cameras on a circle
 * around the small sphere, all rendered in ONE kernel launch on one MI355X -- written as turntable_<v>.ppm.
 *   gcc -std=c99 -Iinclude examples/render_batch_c.c -Lraytracingweekend.jl_amd/lib -lrtw_hip -Wl,-rpath,$PWD/raytracingweekend.jl_amd/lib -lm -o render_batch_c
 *   ./render_batch_c [width 400] [spp 16] [views 8]
 * tests/test_batch_abi.py compiles and links it (no GPU needed for that); running it needs a GPU. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "rtw_hip.h"

/* Camera(lookfrom, lookat, vup = (0,1,0), vfov = 90, aspect 16/9, aperture 0, focus 1) (src/camera.jl:18-36) */
static rtw_camera_f32 look_at(const float from[3], const float at[3]) {
    const float h = 1.0f, vh = 2.0f * h, vw = 16.0f / 9.0f * vh;       /* tan(vfov / 2) = 1 */
    float w[3] = {from[0] - at[0], from[1] - at[1], from[2] - at[2]};
    float n = sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    for (int k = 0; k < 3; ++k) w[k] /= n;
    float u[3] = {w[2], 0.0f, -w[0]};                                   /* cross((0,1,0), w) */
    n = sqrtf(u[0] * u[0] + u[2] * u[2]);
    u[0] /= n; u[2] /= n;
    const float v[3] = {w[1] * u[2] - w[2] * u[1], w[2] * u[0] - w[0] * u[2], w[0] * u[1] - w[1] * u[0]};   /* cross(w, u) */
    rtw_camera_f32 c;
    for (int k = 0; k < 3; ++k) {
        c.origin[k] = from[k];
        c.horizontal[k] = vw * u[k];
        c.vertical[k] = vh * v[k];
        c.lower_left_corner[k] = from[k] - c.horizontal[k] / 2 - c.vertical[k] / 2 - w[k];
        c.u[k] = u[k]; c.v[k] = v[k]; c.w[k] = w[k];
    }
    c.lens_radius = 0.0f;
    return c;
}

int main(int argc, char **argv) {
    const int width = argc > 1 ? atoi(argv[1]) : 400, spp = argc > 2 ? atoi(argv[2]) : 16, n = argc > 3 ? atoi(argv[3]) : 8;
    const int height = width * 9 / 16;
    if (width <= 0 || height <= 0 || spp <= 0 || n <= 0) return 2;
    const float cx[2] = {0.0f, 0.0f}, cy[2] = {0.0f, -100.5f}, cz[2] = {-1.0f, -1.0f}, r[2] = {0.5f, 100.0f};
    const int32_t kind[2] = {RTW_LAMBERTIAN, RTW_LAMBERTIAN};
    const float ar[2] = {0.7f, 0.8f}, ag[2] = {0.3f, 0.8f}, ab[2] = {0.3f, 0.0f}, param[2] = {0.0f, 0.0f};
    rtw_scene_f32 scene = {2, cx, cy, cz, r, kind, ar, ag, ab, param};
    rtw_camera_f32 *cams = (rtw_camera_f32 *)malloc((size_t)n * sizeof *cams);
    uint64_t *seeds = (uint64_t *)malloc((size_t)n * sizeof *seeds);
    float *img = (float *)malloc((size_t)n * width * height * 3 * sizeof(float));
    if (!cams || !seeds || !img) return 2;
    const float at[3] = {0.0f, 0.0f, -1.0f};
    for (int v = 0; v < n; ++v) {
        const float a = 6.2831853f * (float)v / (float)n;
        const float from[3] = {2.0f * sinf(a), 0.5f, -1.0f + 2.0f * cosf(a)};
        cams[v] = look_at(from, at);
        seeds[v] = 1;
    }
    rtw_params p = {0};
    p.width = width; p.height = height; p.spp = spp; p.max_depth = 16; p.seed = 1;
    p.shard_count = 1; p.device = -1; p.gamma = 1;
    if (rtw_abi_version() != RTW_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 2; }
    int rc = rtw_render_batch_f32(&scene, cams, n, seeds, &p, img);
    if (rc) { fprintf(stderr, "rtw_render_batch_f32: %d: %s\n", rc, rtw_last_error()); return 1; }
    rtw_stats_t st;
    if (rtw_stats(&st) == 0) fprintf(stderr, "%d views: %llu samples, %llu segments, kernel %.3f ms\n", n, (unsigned long long)st.samples, (unsigned long long)st.segments, st.kernel_ms);
    for (int v = 0; v < n; ++v) {
        char name[64];
        snprintf(name, sizeof name, "turntable_%03d.ppm", v);
        FILE *f = fopen(name, "wb");
        if (!f) return 2;
        fprintf(f, "P6\n%d %d\n255\n", width, height);
        const float *frame = img + (size_t)v * width * height * 3;         /* view v: the v-th consecutive Matrix{RGB{T}} */
        for (int i = 0; i < height; ++i)
            for (int j = 0; j < width; ++j)
                for (int c = 0; c < 3; ++c) {
                    float x = frame[((size_t)j * height + i) * 3 + c];
                    x = x < 0 ? 0 : (x > 1 ? 1 : x);
                    fputc((int)lrintf(x * 255.0f), f);
                }
        fclose(f);
    }
    free(img); free(seeds); free(cams);
    rtw_shutdown();
    return 0;
}
