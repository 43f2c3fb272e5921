/* A focus bracket from C (include/rtw_hip.h rtw_lens_batch_f32 with n_frames == 1): the two-sphere scene is rendered ONCE through the
 * pinhole, its feature pass runs once, and five focus distances are applied to that one frame in ONE call -- six launches for all five
 * lenses, one copy back -- into focus_0.ppm .. focus_4.ppm.
 *   gcc -std=c99 -Iinclude examples/render_focus_bracket_c.c -Lraytracingweekend.jl_amd/lib -lrtw_hip -Wl,-rpath,$PWD/raytracingweekend.jl_amd/lib -lm -o render_focus_bracket_c
 *   ./render_focus_bracket_c [width 400] [spp 4]
 * tests/test_lens_batch_abi.py compiles and links it (no GPU needed for that); running it needs a GPU. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rtw_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s: %d: %s\n", #call, rc_, rtw_last_error()); return 1; } } while (0)
#define N_LENSES 5

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
    /* a pinhole at the origin looking down -z, vfov 90, 16:9: the viewport one unit in front of the eye */
    rtw_camera_f32 cam;
    memset(&cam, 0, sizeof cam);
    const float vh = 2.0f, vw = 16.0f / 9.0f * vh;
    cam.horizontal[0] = vw; cam.vertical[1] = vh;
    cam.lower_left_corner[0] = -vw / 2; cam.lower_left_corner[1] = -vh / 2; cam.lower_left_corner[2] = -1.0f;
    cam.u[0] = 1.0f; cam.v[1] = 1.0f; cam.w[2] = 1.0f;
    cam.lens_radius = 0.0f;
    rtw_params p;
    memset(&p, 0, sizeof p);
    p.width = width; p.height = height; p.spp = spp; p.max_depth = 16; p.seed = 1;
    p.shard_count = 1; p.device = -1; p.gamma = 0;             /* linear: the lens stage applies the gamma */
    rtw_wide_aperture_t b;
    memset(&b, 0, sizeof b);
    b.max_radius = RTW_WIDE_APERTURE_MAX_RADIUS; b.gamma = 1; b.device = -1;
    b.lens_radius = 0.05;                                      /* one aperture for the whole bracket: K = 0.05 * width / 3.56 */
    const double focus[N_LENSES] = {0.5, 0.75, 1.0, 2.0, 8.0};  /* the sphere's front is 0.5 away, the horizon far behind it */
    rtw_camera_f32 cams[N_LENSES];
    for (int v = 0; v < N_LENSES; ++v) cams[v] = cam;          /* one camera under five lenses */
    if (rtw_abi_version() != RTW_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 2; }
    const size_t n_pix = (size_t)width * height;
    float *image = (float *)malloc(n_pix * 3 * sizeof(float)), *features = (float *)malloc(n_pix * RTW_FEATURE_CHANNELS * sizeof(float));
    float *out = (float *)malloc(N_LENSES * n_pix * 3 * sizeof(float));
    if (!image || !features || !out) return 2;

    CHECK(rtw_render_f32(&scene, &cam, &p, image));            /* ONE render ... */
    rtw_stats_t st;
    CHECK(rtw_stats(&st));
    CHECK(rtw_render_features_f32(&scene, &cam, &p, 0, 0, features));       /* ... ONE feature pass over all chunks ... */
    CHECK(rtw_lens_batch_f32(&b, cams, N_LENSES, 1 /* n_frames: every lens reads the one frame */, NULL /* b.lens_radius for all */, focus, width, height, image,
                             features, out));                  /* ... and five lenses in one call */
    fprintf(stderr, "%d x %d at %d spp: trace kernel %.3f ms, then %d focus distances in one call\n", width, height, spp, st.kernel_ms, N_LENSES);
    for (int v = 0; v < N_LENSES; ++v) {
        char name[32];
        sprintf(name, "focus_%d.ppm", v);
        if (write_ppm(name, width, height, out + (size_t)v * n_pix * 3)) return 2;
    }
    free(image); free(features); free(out);
    rtw_shutdown();
    return 0;
}
