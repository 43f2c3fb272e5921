/* Ray queries from C (include/rtw_hip.h rtw_cast_rays_f32): the intersection routine itself, without a frame.  Picks the sphere of the
 * two-sphere scene under a few screen positions that are no pixel centres -- index, distance, hit point and normal --, then tests two
 * shadow rays between a point on the ground and two lights: a ray from the point towards the light with tmax = their distance and no
 * record (rec == NULL) is occluded exactly when it hits anything.
 *   gcc -std=c99 -Iinclude examples/cast_rays_c.c -Lraytracingweekend.jl_amd/lib -lrtw_hip -Wl,-rpath,$PWD/raytracingweekend.jl_amd/lib -lm -o cast_rays_c
 *   ./cast_rays_c
 * tests/test_rays_abi.py compiles and links it (no GPU needed for that); running it needs a GPU. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "rtw_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s: %d: %s\n", #call, rc_, rtw_last_error()); return 1; } } while (0)

/* a ray from `from` towards `to`: unit direction, tmax as given (INFINITY: unbounded; negative: the distance between the points) */
static void ray_between(float *ray, const float from[3], const float to[3], float tmax, float tag) {
    float d[3], len = 0.0f;
    for (int k = 0; k < 3; ++k) { d[k] = to[k] - from[k]; len += d[k] * d[k]; }
    len = sqrtf(len);
    for (int k = 0; k < 3; ++k) { ray[k] = from[k]; ray[3 + k] = d[k] / len; }
    ray[6] = tmax < 0.0f ? len : tmax;
    ray[7] = tag;
}

int main(void) {
    const float cx[2] = {0.0f, 0.0f}, cy[2] = {0.0f, -100.5f}, cz[2] = {-1.0f, -1.0f}, r[2] = {0.5f, 100.0f};
    const int32_t kind[2] = {RTW_LAMBERTIAN, RTW_LAMBERTIAN};
    const float ar[2] = {0.7f, 0.8f}, ag[2] = {0.3f, 0.8f}, ab[2] = {0.3f, 0.0f}, param[2] = {0.0f, 0.0f};
    rtw_scene_f32 scene = {2, cx, cy, cz, r, kind, ar, ag, ab, param};
    if (rtw_abi_version() != RTW_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 2; }
    rtw_rays_params p;
    memset(&p, 0, sizeof p);
    p.device = -1;
    p.tmin = 1e-4;                                  /* the reference's */

    /* picking: default_camera((0,0,0), (0,0,-1), (0,1,0), 90, 16/9, 0, 1) (src/camera.jl:18-36) -- the viewport is 32/9 x 2 at z = -1 */
    const float eye[3] = {0.0f, 0.0f, 0.0f}, vw = 32.0f / 9.0f, vh = 2.0f;
    const float screen[4][2] = {{0.5f, 0.5f}, {0.37f, 0.52f}, {0.5f, 0.1f}, {0.013f, 0.97f}};      /* (s, t) in [0, 1]^2, t upwards */
    enum { N_PICK = 4 };
    float rays[N_PICK * 8], rec[N_PICK * 8];
    int32_t idx[N_PICK];
    for (int k = 0; k < N_PICK; ++k) {
        const float at[3] = {-vw / 2 + screen[k][0] * vw, -vh / 2 + screen[k][1] * vh, -1.0f};
        ray_between(rays + 8 * k, eye, at, INFINITY, (float)k);
    }
    CHECK(rtw_cast_rays_f32(&scene, rays, N_PICK, &p, idx, rec));
    rtw_stats_t st;
    CHECK(rtw_stats(&st));
    for (int k = 0; k < N_PICK; ++k) {
        const float *h = rec + 8 * k;
        if (idx[k] < 0) printf("screen (%.3f, %.3f): nothing\n", screen[k][0], screen[k][1]);
        else printf("screen (%.3f, %.3f): sphere %d at t = %.4f, p = (%.3f, %.3f, %.3f), n = (%.3f, %.3f, %.3f), %s face\n", screen[k][0], screen[k][1], (int)idx[k],
                    h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7] != 0.0f ? "front" : "back");
    }
    fprintf(stderr, "%llu rays, %llu sphere tests, kernel %.3f ms\n", (unsigned long long)st.segments, (unsigned long long)st.sphere_tests, st.kernel_ms);

    /* shadow rays: is the light visible from a point just above the ground?  tmax = the distance, no records */
    const float point[3] = {0.8f, -0.49f, -1.0f}, lights[2][3] = {{-2.0f, 1.5f, -1.0f}, {2.0f, 1.5f, -1.0f}};
    float shadow[2 * 8];
    int32_t blocker[2];
    for (int k = 0; k < 2; ++k) ray_between(shadow + 8 * k, point, lights[k], -1.0f, (float)k);
    CHECK(rtw_cast_rays_f32(&scene, shadow, 2, &p, blocker, NULL));
    for (int k = 0; k < 2; ++k) {
        if (blocker[k] < 0) printf("light %d at (%.1f, %.1f, %.1f): visible\n", k, lights[k][0], lights[k][1], lights[k][2]);
        else printf("light %d at (%.1f, %.1f, %.1f): in the shadow of sphere %d\n", k, lights[k][0], lights[k][1], lights[k][2], (int)blocker[k]);
    }
    rtw_shutdown();
    return 0;
}
