/* Adaptive sampling from C (include/rtw_hip.h rtw_render_adaptive_f32): the two-sphere scene rendered until every 8x8 tile passes the
 * stopping rule at `tolerance` or holds all `spp` samples; then refined to half the tolerance on the same accumulator.  Prints how many
 * tiles stopped where and the share of the uniform render's samples that was spent, and checks one tile against the prefix render the
 * contract names (rtw_render_f32 with spp = the samples the tile holds, n_chunks = its chunk count).  Writes adaptive.ppm.
 *   gcc -std=c99 -Iinclude examples/render_adaptive_c.c -Lraytracingweekend.jl_amd/lib -lrtw_hip -Wl,-rpath,$PWD/raytracingweekend.jl_amd/lib -lm -o render_adaptive_c
 *   ./render_adaptive_c [width 400] [spp 256] [tolerance 0.05]
 * tests/test_adaptive_abi.py compiles and links it (no GPU needed for that); running it needs a GPU. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rtw_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s: %d: %s\n", #call, rc_, rtw_last_error()); return 1; } } while (0)

int main(int argc, char **argv) {
    const int width = argc > 1 ? atoi(argv[1]) : 400, spp = argc > 2 ? atoi(argv[2]) : 256;
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
    const size_t n = (size_t)width * height * 3;
    float *img = (float *)malloc(n * sizeof(float)), *ref = (float *)malloc(n * sizeof(float));
    if (!img || !ref) return 2;

    rtw_scene_handle sc;
    rtw_accum_handle acc;
    CHECK(rtw_scene_upload_f32(&scene, -1, &sc));
    CHECK(rtw_accum_create(-1, width, height, &acc));
    rtw_adaptive_info_t info;
    rtw_accum_info_t ai;
    for (int step = 0; step < 2; ++step) {                      /* the second call refines: same accumulator, half the tolerance */
        CHECK(rtw_render_adaptive_f32(sc, &cam, &p, &ad, acc, NULL, NULL));
        CHECK(rtw_accum_adaptive_info(acc, &info));
        fprintf(stderr, "tolerance %g: %d passes; %d of %d tiles stopped by the rule, %d hold all chunks; chunks per tile %d .. %d; %.1f %% of %d spp\n",
                info.tolerance, info.rounds, info.tiles_converged, info.n_tiles, info.tiles_at_cap, info.min_chunks_held, info.max_chunks_held,
                100.0 * (double)info.samples / ((double)width * height * spp), spp);
        ad.tolerance *= 0.5;
    }
    CHECK(rtw_accum_resolve_host_f32(acc, 1, img));
    CHECK(rtw_accum_info(acc, &ai));
    /* tile 0 (rows 0..7, column strip 0..7) is the render of the prefix it holds */
    int32_t n_tiles = 0, c0 = 0;
    CHECK(rtw_accum_tile_chunks(acc, 1, &n_tiles, &c0));
    rtw_params q = p;
    q.n_chunks = c0;
    q.spp = c0 * ai.chunk_spp < spp ? c0 * ai.chunk_spp : spp;
    CHECK(rtw_render_f32(&scene, &cam, &q, ref));
    for (int j = 0; j < 8 && j < width; ++j)
        for (int i = 0; i < 8 && i < height; ++i)
            if (memcmp(&img[((size_t)j * height + i) * 3], &ref[((size_t)j * height + i) * 3], 3 * sizeof(float)) != 0) {
                fprintf(stderr, "tile 0 differs from the render of its %d chunks\n", c0);
                return 3;
            }
    fprintf(stderr, "tile 0 == the render of %d spp in %d chunks\n", q.spp, c0);
    CHECK(rtw_accum_free(acc));
    CHECK(rtw_scene_free(sc));
    FILE *f = fopen("adaptive.ppm", "wb");
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
    free(img); free(ref);
    rtw_shutdown();
    return 0;
}
