/* Radiance queries from C (include/rtw_hip.h rtw_trace_rays_f32): a radiance probe.  From one point above the ground of the two-sphere
 * scene, 384 directions spread evenly over the sphere (a Fibonacci spiral), 64 samples of ray_color each -- no camera, no pixels.  Prints
 * the mean radiance of the upper and of the lower hemisphere and of the whole probe (what an irradiance probe or a light baker would go
 * on to weight with a cosine or with spherical harmonics), then traces the same list in two calls with first_stream advanced and checks
 * that the words are those of the one call.
 *   gcc -std=c99 -Iinclude examples/trace_rays_c.c -Lraytracingweekend.jl_amd/lib -lrtw_hip -Wl,-rpath,$PWD/raytracingweekend.jl_amd/lib -lm -o trace_rays_c
 *   ./trace_rays_c
 * tests/test_trace_rays_abi.py compiles and links it (no GPU needed for that); running it needs a GPU. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "rtw_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s: %d: %s\n", #call, rc_, rtw_last_error()); return 1; } } while (0)

enum { N_DIR = 384, SPP = 64 };

int main(void) {
    const float cx[2] = {0.0f, 0.0f}, cy[2] = {0.0f, -100.5f}, cz[2] = {-1.0f, -1.0f}, r[2] = {0.5f, 100.0f};
    const int32_t kind[2] = {RTW_LAMBERTIAN, RTW_LAMBERTIAN};
    const float ar[2] = {0.7f, 0.8f}, ag[2] = {0.3f, 0.8f}, ab[2] = {0.3f, 0.0f}, param[2] = {0.0f, 0.0f};
    rtw_scene_f32 scene = {2, cx, cy, cz, r, kind, ar, ag, ab, param};
    if (rtw_abi_version() != RTW_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 2; }
    rtw_trace_params p;
    memset(&p, 0, sizeof p);
    p.device = -1;
    p.spp = SPP;
    p.max_depth = 16;
    p.seed = 1;

    /* the probe: 0.3 above the ground, beside the small sphere */
    static float rays[N_DIR * 8];
    static double out[N_DIR * 3], split[N_DIR * 3];
    const double golden = 3.14159265358979323846 * (3.0 - sqrt(5.0));
    for (int k = 0; k < N_DIR; ++k) {
        const double y = 1.0 - (2.0 * k + 1.0) / N_DIR, rad = sqrt(1.0 - y * y), phi = golden * k;
        float *q = rays + 8 * k;
        q[0] = 0.9f; q[1] = -0.2f; q[2] = -1.0f;
        q[3] = (float)(rad * cos(phi)); q[4] = (float)y; q[5] = (float)(rad * sin(phi));
        q[6] = INFINITY; q[7] = (float)k;                  /* not read by this call: the list serves rtw_cast_rays_f32 as it is */
    }
    CHECK(rtw_trace_rays_f32(&scene, rays, N_DIR, &p, out));
    rtw_stats_t st;
    CHECK(rtw_stats(&st));
    double up[3] = {0, 0, 0}, down[3] = {0, 0, 0};
    for (int k = 0; k < N_DIR; ++k)
        for (int c = 0; c < 3; ++c) (rays[8 * k + 4] > 0.0f ? up : down)[c] += out[3 * k + c];
    printf("probe at (0.9, -0.2, -1.0), %d directions x %d samples\n", (int)N_DIR, (int)SPP);
    printf("  upper hemisphere: mean radiance (%.4f, %.4f, %.4f)\n", up[0] / (N_DIR / 2), up[1] / (N_DIR / 2), up[2] / (N_DIR / 2));
    printf("  lower hemisphere: mean radiance (%.4f, %.4f, %.4f)\n", down[0] / (N_DIR / 2), down[1] / (N_DIR / 2), down[2] / (N_DIR / 2));
    printf("  all directions:   mean radiance (%.4f, %.4f, %.4f)\n", (up[0] + down[0]) / N_DIR, (up[1] + down[1]) / N_DIR, (up[2] + down[2]) / N_DIR);
    fprintf(stderr, "%llu samples, %llu segments (%.2f per sample), kernel %.3f ms\n", (unsigned long long)st.samples, (unsigned long long)st.segments,
            (double)st.segments / (double)st.samples, st.kernel_ms);

    /* the same list in two calls: the second with first_stream advanced by the first call's n */
    const int64_t first = 100;
    CHECK(rtw_trace_rays_f32(&scene, rays, first, &p, split));
    p.first_stream = (uint64_t)first;
    CHECK(rtw_trace_rays_f32(&scene, rays + 8 * first, N_DIR - first, &p, split + 3 * first));
    if (memcmp(out, split, sizeof out) != 0) { fprintf(stderr, "the two calls differ from the one call\n"); return 1; }
    printf("traced in two calls: the same words\n");
    rtw_shutdown();
    return 0;
}
