/* A display-ready frame from C (include/rtw_hip.h rtw_render_presented_f32): configs[0] -- the two-sphere scene, 96 x 54 at 16 samples per
 * pixel, depth 4 -- rendered and presented in one call.  The bytes that come back are the rows of the PPM: this example writes them as they
 * are; it neither clamps nor rounds nor transposes on the host.
 *   gcc -std=c99 -Iinclude examples/render_presented_c.c -Lraytracingweekend.jl_amd/lib -lrtw_hip -Wl,-rpath,$PWD/raytracingweekend.jl_amd/lib -lm -o render_presented_c
 *   ./render_presented_c [width 96] [spp 16]
 * tests/test_present_abi.py compiles and links it (no GPU needed for that); running it needs a GPU. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rtw_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s: %d: %s\n", #call, rc_, rtw_last_error()); return 1; } } while (0)

int main(int argc, char **argv) {
    const int width = argc > 1 ? atoi(argv[1]) : 96, spp = argc > 2 ? atoi(argv[2]) : 16;
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
    rtw_params params;
    memset(&params, 0, sizeof params);
    params.width = width; params.height = height; params.spp = spp; params.max_depth = 4; params.seed = 1;
    params.shard_count = 1; params.device = -1; params.gamma = 1;
    rtw_present_t p;
    memset(&p, 0, sizeof p);
    p.channels = 3; p.device = -1; p.exposure = 1.0;          /* no flags, NaN -> black: the 8-bit image imageio.to_u8 defines */
    if (rtw_abi_version() != RTW_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 2; }
    const int64_t bytes = rtw_present_bytes(width, height, p.channels, 0);
    if (bytes < 0) { fprintf(stderr, "rtw_present_bytes: %d: %s\n", (int)bytes, rtw_last_error()); return 1; }
    uint8_t *rows = (uint8_t *)malloc((size_t)bytes);
    if (!rows) return 2;

    CHECK(rtw_render_presented_f32(&scene, &cam, &params, NULL /* no filter */, &p, rows));
    rtw_stats_t st;
    CHECK(rtw_stats(&st));
    fprintf(stderr, "%d x %d at %d spp: trace kernel %.3f ms; %ld bytes came back instead of %ld\n", width, height, spp, st.kernel_ms, (long)bytes,
            (long)((size_t)width * height * 3 * sizeof(float)));
    FILE *f = fopen("render_presented_c.ppm", "wb");
    if (!f) return 2;
    fprintf(f, "P6\n%d %d\n255\n", width, height);
    if (fwrite(rows, 1, (size_t)bytes, f) != (size_t)bytes) return 2;
    fclose(f);
    free(rows);
    rtw_shutdown();
    return 0;
}
