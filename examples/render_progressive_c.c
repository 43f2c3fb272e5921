/* Progressive render from C (include/rtw_hip.h rtw_render_accum_f32): the two-sphere scene rendered in passes into an exact
 * accumulator -- exported after the second pass, freed, imported again (the checkpoint) and finished -- then compared with the
 * one-shot rtw_render_f32 of the same frame by memcmp: the two images are the same bytes.  Writes progressive.ppm.
 *   gcc -std=c99 -Iinclude examples/render_progressive_c.c -Lraytracingweekend.jl_amd/lib -lrtw_hip -Wl,-rpath,$PWD/raytracingweekend.jl_amd/lib -lm -o render_progressive_c
 *   ./render_progressive_c [width 400] [spp 64] [passes 4]
 * tests/test_accum_abi.py compiles and links it (no GPU needed for that); running it needs a GPU. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rtw_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s: %d: %s\n", #call, rc_, rtw_last_error()); return 1; } } while (0)

int main(int argc, char **argv) {
    const int width = argc > 1 ? atoi(argv[1]) : 400, spp = argc > 2 ? atoi(argv[2]) : 64;
    int passes = argc > 3 ? atoi(argv[3]) : 4;
    const int height = width * 9 / 16;
    if (width <= 0 || height <= 0 || spp <= 0 || passes <= 0) return 2;
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
    const size_t n = (size_t)width * height * 3;
    float *one_shot = (float *)malloc(n * sizeof(float)), *img = (float *)malloc(n * sizeof(float));
    if (!one_shot || !img) return 2;

    rtw_scene_handle sc;
    rtw_accum_handle acc;
    CHECK(rtw_scene_upload_f32(&scene, -1, &sc));
    CHECK(rtw_accum_create(-1, width, height, &acc));
    const int n_chunks = spp < 256 ? spp : 256;                 /* the default rule of rtw_params.n_chunks: here 1 sample per chunk up to 256 */
    const int chunk_spp = (spp + n_chunks - 1) / n_chunks, n_eff = (spp + chunk_spp - 1) / chunk_spp;
    if (passes > n_eff) passes = n_eff;
    for (int k = 0; k < passes; ++k) {
        const int begin = (int)((long long)k * n_eff / passes), end = (int)((long long)(k + 1) * n_eff / passes);
        CHECK(rtw_render_accum_f32(sc, &cam, &p, begin, end - begin, acc, NULL, NULL));
        rtw_accum_info_t info;
        CHECK(rtw_accum_info(acc, &info));
        fprintf(stderr, "pass %d: chunks [%d, %d), %d of %d samples\n", k + 1, begin, end, info.samples_done, info.spp);
        if (k == 1) {                                           /* checkpoint: export, free, import, go on */
            uint64_t size = 0;
            CHECK(rtw_accum_export(acc, NULL, 0, &size));
            void *blob = malloc((size_t)size);
            if (!blob) return 2;
            CHECK(rtw_accum_export(acc, blob, size, &size));
            CHECK(rtw_accum_free(acc));
            CHECK(rtw_accum_import(-1, blob, size, &acc));
            free(blob);
            fprintf(stderr, "checkpoint: %llu bytes exported and imported\n", (unsigned long long)size);
        }
    }
    CHECK(rtw_accum_resolve_host_f32(acc, 1, img));
    CHECK(rtw_accum_free(acc));
    CHECK(rtw_scene_free(sc));
    CHECK(rtw_render_f32(&scene, &cam, &p, one_shot));
    if (memcmp(img, one_shot, n * sizeof(float)) != 0) { fprintf(stderr, "the progressive image differs from the one-shot render\n"); return 3; }
    fprintf(stderr, "%d passes == one render of %d spp: %zu bytes identical\n", passes, spp, n * sizeof(float));
    FILE *f = fopen("progressive.ppm", "wb");
    if (!f) return 2;
    fprintf(f, "P6\n%d %d\n255\n", width, height);
    for (int i = 0; i < height; ++i)
        for (int j = 0; j < width; ++j)
            for (int c = 0; c < 3; ++c) {
                float x = img[((size_t)j * height + i) * 3 + c];
                x = x < 0 ? 0 : (x > 1 ? 1 : x);
                fputc((int)lrintf(x * 255.0f), f);
            }
    fclose(f);
    free(img); free(one_shot);
    rtw_shutdown();
    return 0;
}
