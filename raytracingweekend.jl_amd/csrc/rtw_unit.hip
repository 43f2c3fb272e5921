// rtw_unit.hip -- the T0 unit entry points (rtw_unit_f32/_f64): host slots -> device -> unit_kernel (rtw_units.hpp) -> host slots
// Per-item ops with a scene: 8 - 11, 13, 14, 26 (scans and the bounce), 17 - 20 (candidate sinks, rows of RTW_SINK_SLOTS slots, scenes of at most
// RTW_SINK_SPHERES spheres), 27 (op 20's sink plus the block vote: rows of RTW_VOTE_SLOTS slots), 28 (the cull layout: item p = device position p;
// the caller's index or -1, in-lane, positions, blocks), 32 - 35 (ops 17 - 20 plus a flush counter: rows of RTW_FLUSH_SLOTS slots, the last one a raw
// uint64 of four 16-bit counts of early resolves -- bits 0-15 A, 16-31 B, 32-47 C of hit_world_mfma (ops 34, 35), bits 48-63 D of hit_world (op 32) or E
// of hit_world_cull (op 33); RTW_FLUSH_* in rtw_scan.hpp).  24 and 29 are not ops; 36 is the first number behind the last op.
#include "rtw_scene_view.hpp"
#include "rtw_units.hpp"

namespace rtwh {

// T0 unit entry point: host slots -> device -> unit_kernel -> host slots
template <typename T, typename SceneT, typename CamT>
int run_unit(int op_arg, int count, const void *in, void *out, const SceneT *scene, const CamT *cam) {
    const int op = op_arg & 0xff, numerics = (op_arg >> 8) & 3;      // bits 8-9: the numerics mode of the ray-sphere test
    if (op_arg < 0 || (op_arg >> 10) != 0 || op >= rtw::U_NUM_OPS || op == 24 || op == 29) return fail(-2, "unknown unit op %d", op_arg);
    if (numerics == 2) return fail(-2, "unknown numerics mode %d (unit op %d)", numerics, op_arg);
    if (rtw::unit_is_accum(op)) return accum_unit(op, sizeof(T) == 8, count, in, out);      // (ops 21-23, 25, 30 and 31: layouts of their own, no scene, no numerics mode)
    if (count < 0 || (count > 0 && (!in || !out))) return fail(-1, "null argument");
    if (count == 0) return 0;
    const bool sink = rtw::unit_is_sink(op);
    const int sop = rtw::unit_sink_of(op);       // (a flush op runs its sink op's scan on the same buffers)
    const bool needs_scene = op == rtw::U_HIT_WORLD || op == rtw::U_RAY_COLOR || op == rtw::U_HIT_WORLD_LDS || op == rtw::U_HIT_WORLD_CULL || op == rtw::U_HIT_WORLD_MFMA || op == rtw::U_HIT_WORLD_MFMA_CULL || op == rtw::U_SHADE || op == rtw::U_CULL_LAYOUT || sink;
    if (needs_scene && !scene) return fail(-1, "op %d needs a scene", op);
    if (sink && scene->n > RTW_SINK_SPHERES) return fail(-5, "unit op %d: the candidate sets hold %d spheres, the scene has %d", op, RTW_SINK_SPHERES, scene->n);
    if (op == rtw::U_GET_RAY && !cam) return fail(-1, "op %d needs a camera", op);
    DeviceGuard guard;
    int dev;
    if (int rc = resolve_device(-1, &dev)) return rc;
    CtxPtr ctx;
    if (int rc = get_ctx(dev, &ctx)) return rc;
    rtw_scene_handle h_raw = nullptr;
    rtw::DevScene<T> S;
    memset(&S, 0, sizeof S);
    rtw::CullScene<T> CS;
    memset(&CS, 0, sizeof CS);
    if (needs_scene) {
        if (int rc = upload_scene<T>(scene, dev, &h_raw)) return rc;
        S = dev_scene_of<T>(h_raw);
        CS = cull_scene_of<T>(h_raw);
    }
    S.numerics = numerics; CS.numerics = numerics;
    ScenePtr h(h_raw);
    HIP_TRY(hipSetDevice(dev));
    rtw::Camera<T> C;
    memset(&C, 0, sizeof C);
    if (cam) C = device_camera<T>(*cam);
    using V4 = typename rtw::Vec4<T>::type;
    size_t lds_bytes = 0;
    if (op == rtw::U_HIT_WORLD_LDS || op == rtw::U_HIT_WORLD_MFMA || sop == rtw::U_SINK_LDS || sop == rtw::U_SINK_MFMA) lds_bytes = (size_t)rtw::scene_geom_alloc(S.n, S.n_pad) * sizeof(V4);
    if ((op == rtw::U_HIT_WORLD_MFMA || sop == rtw::U_SINK_MFMA) && !S.mf_ops) return fail(-5, "the scene has no matrix-pipe scan operands (unit op %d)", op);
    if ((op == rtw::U_HIT_WORLD_MFMA_CULL || sop == rtw::U_SINK_MFMA_CULL || op == rtw::U_SINK_MFMA_CULL_VOTE || op == rtw::U_CULL_LAYOUT) && !CS.mf_ops) return fail(-5, "the scene has no matrix-pipe cull operands (unit op %d)", op);
    if (op == rtw::U_HIT_WORLD_CULL || op == rtw::U_HIT_WORLD_MFMA_CULL || sop == rtw::U_SINK_CULL || sop == rtw::U_SINK_MFMA_CULL || op == rtw::U_SINK_MFMA_CULL_VOTE) {
        const size_t n_cull = (size_t)rtw::cull_exact_count(CS);
        lds_bytes = n_cull * sizeof(V4) + ((n_cull * sizeof(unsigned short) + 15) / 16) * 16;
    }
    if (lds_bytes > 60 * 1024) return fail(-5, "scene too large for the LDS-staged unit op %d (%zu bytes)", op, lds_bytes);
    const size_t in_b = (size_t)count * rtw::unit_in_slots(op) * 8, out_b = (size_t)count * rtw::unit_out_slots(op) * 8;
    double *d_in = nullptr, *d_out = nullptr;
    int rc = 0;
    hipError_t e;
    if ((e = hipMalloc(&d_in, in_b)) != hipSuccess || (e = hipMalloc(&d_out, out_b)) != hipSuccess ||
        (e = hipMemcpy(d_in, in, in_b, hipMemcpyHostToDevice)) != hipSuccess || (sink && (e = hipMemset(d_out, 0, out_b)) != hipSuccess)) {
        rc = fail((int)e, "unit buffers: %s", hipGetErrorString(e));
    } else {
        (void)hipGetLastError();
        hipLaunchKernelGGL(rtw::unit_kernel<T>, dim3((count + 63) / 64), dim3(64), lds_bytes, 0, op, count, d_in, d_out, S, CS, C);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipMemcpy(out, d_out, out_b, hipMemcpyDeviceToHost)) != hipSuccess)
            rc = fail((int)e, "unit kernel: %s", hipGetErrorString(e));
    }
    if (d_in) HIP_IGNORE(hipFree(d_in));
    if (d_out) HIP_IGNORE(hipFree(d_out));
    return rc;
}

template int run_unit<float>(int, int, const void *, void *, const rtw_scene_f32 *, const rtw_camera_f32 *);
template int run_unit<double>(int, int, const void *, void *, const rtw_scene_f64 *, const rtw_camera_f64 *);

}  // namespace rtwh
