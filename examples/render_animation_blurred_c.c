/* An animation with history reuse AND motion blur from C (include/rtw_hip.h rtw_render_blurred_f32): the scene of render_animation_c.c -- a
 * small sphere rolls over the ground past a resting one -- rendered by ONE call that, behind every frame's step, blurs the frame along the
 * motion plane: the velocity and tile-max launch, the neighbour-max launch and the gather.  Frame 0 has no previous camera and passes
 * through.  Frame v is written to blurred_<v>.ppm.  With a fourth argument 0 the blur is left out (rtw_render_animation_f32): compare the
 * rolling sphere's edges.
 *   gcc -std=c99 -Iinclude examples/render_animation_blurred_c.c -Lraytracingweekend.jl_amd/lib -lrtw_hip -Wl,-rpath,$PWD/raytracingweekend.jl_amd/lib -lm -o render_animation_blurred_c
 *   ./render_animation_blurred_c [width 96] [spp 1] [frames 8] [blur 1] [shutter 1.0]
 * tests/test_motion_blur_abi.py compiles and links it (no GPU needed for that); running it needs a GPU. */
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
    const int width = argc > 1 ? atoi(argv[1]) : 96, spp = argc > 2 ? atoi(argv[2]) : 1, frames = argc > 3 ? atoi(argv[3]) : 8;
    const int blur_on = argc > 4 ? atoi(argv[4]) : 1;
    const double shutter = argc > 5 ? atof(argv[5]) : 1.0;
    const int height = width * 9 / 16;
    if (width <= 0 || height <= 0 || spp <= 0 || frames <= 0 || frames > 4096) return 2;
    /* one scene per frame.  Sphere 0 rolls along x, the others rest: the frames share every array but cx. */
    float (*cx)[3] = malloc((size_t)frames * sizeof *cx);
    rtw_scene_f32 *scenes = malloc((size_t)frames * sizeof *scenes);
    rtw_camera_f32 *cams = malloc((size_t)frames * sizeof *cams);
    uint64_t *seeds = malloc((size_t)frames * sizeof *seeds);
    if (!cx || !scenes || !cams || !seeds) return 3;
    const float cy[3] = {-0.2f, 0.0f, -100.5f}, cz[3] = {-1.0f, -1.6f, -1.0f}, r[3] = {0.3f, 0.5f, 100.0f};
    const int32_t kind[3] = {RTW_LAMBERTIAN, RTW_LAMBERTIAN, RTW_LAMBERTIAN};
    const float ar[3] = {0.8f, 0.3f, 0.8f}, ag[3] = {0.3f, 0.4f, 0.8f}, ab[3] = {0.2f, 0.8f, 0.0f}, param[3] = {0.0f, 0.0f, 0.0f};
    rtw_camera_f32 cam;                                       /* a pinhole camera at the origin looking down -z: vfov 90 degrees, 16:9, focus distance 1 */
    memset(&cam, 0, sizeof cam);
    cam.horizontal[0] = 32.0f / 9.0f; cam.vertical[1] = 2.0f;
    cam.lower_left_corner[0] = -16.0f / 9.0f; cam.lower_left_corner[1] = -1.0f; cam.lower_left_corner[2] = -1.0f;
    cam.u[0] = 1.0f; cam.v[1] = 1.0f; cam.w[2] = 1.0f;
    rtw_params p;
    memset(&p, 0, sizeof p);
    p.width = width; p.height = height; p.spp = spp; p.max_depth = 16;
    p.shard_count = 1; p.device = -1; p.gamma = 1;           /* applied once, by the last stage: the blur, or without it the steps */
    rtw_temporal_t t;                                         /* (the defaults: untuned) */
    memset(&t, 0, sizeof t);
    t.normal_power_log2 = 1; t.flags = RTW_TEMPORAL_DEMODULATE; t.gamma = 1; t.device = -1;
    t.sigma_depth = 0.1; t.min_weight = 0.25; t.history_max = 16.0;
    rtw_velocity_blur_t b;
    memset(&b, 0, sizeof b);
    b.taps = 15; b.gamma = 1; b.device = -1; b.shutter = shutter; b.depth_extent = 0.5;
    if (rtw_abi_version() != RTW_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 2; }
    const size_t n_pix = (size_t)width * height;
    for (int v = 0; v < frames; ++v) {
        cx[v][0] = -1.5f + 3.0f * (float)v / (float)(frames > 1 ? frames - 1 : 1); cx[v][1] = 0.6f; cx[v][2] = 0.0f;
        const rtw_scene_f32 scene = {3, cx[v], cy, cz, r, kind, ar, ag, ab, param};
        scenes[v] = scene; cams[v] = cam; seeds[v] = 1 + (uint64_t)v;
    }
    float *out = malloc((size_t)frames * n_pix * 3 * sizeof(float));
    if (!out) return 3;
    if (blur_on) CHECK(rtw_render_blurred_f32(scenes, cams, frames, seeds, &p, &t, NULL, NULL, &b, out));
    else CHECK(rtw_render_animation_f32(scenes, cams, frames, seeds, &p, &t, NULL, NULL, out));
    for (int v = 0; v < frames; ++v) {
        char name[64];
        snprintf(name, sizeof name, "blurred_%03d.ppm", v);
        if (write_ppm(name, width, height, out + (size_t)v * n_pix * 3)) return 4;
    }
    printf("%d frames of %d x %d at %d spp, blur %s (shutter %.2f, workspace %lld bytes) -> blurred_000.ppm ...\n", frames, width, height, spp, blur_on ? "on" : "off", shutter,
           (long long)rtw_velocity_blur_work_bytes(width, height, 4));
    free(out); free(cx); free(scenes); free(cams); free(seeds);
    rtw_shutdown();
    return 0;
}
