#!/usr/bin/env python3
"""What adaptive sampling costs and buys (include/rtw_hip.h rtw_render_adaptive_*), on one MI355X.
usage: python tools/gpu_adaptive.py [--reps 3] [--tolerances 0.1,0.05,0.03,0.02,0.01] [--out profiles/adaptive_frames.json]

The headline frame (scene_random_spheres, t_cam1, 1920 x 1080, 1000 spp = 250 chunks of 4, depth 50, Float32; default checkpoints: every
32 chunks):
  cost    an adaptive render at an unreachable tolerance (every tile runs to 1000 spp; the frame is checked against the one-shot render)
          against rtw_render_accum_f32 with the SAME pass structure (32 chunks per pass) and against ONE rtw_render_device_f32: wall time
          (host clock, median of --reps, the three alternating within a repetition) and summed HIP-event kernel time.  The difference
          adaptive - accum is one more LDS atomic per channel and sample, the tile lists, and the check kernels with their host waits.
  gain    per tolerance: the samples taken as a share of W x H x 1000, wall ms, passes, the active tiles of every pass, and the RMSE of
          the linear (gamma = 0) image against ONE uniform render of 4000 spp (another seed's samples would do as well: the yardstick
          only has to be much better than what it measures) -- next to the same RMSE of the uniform 1000-spp render.
Every frame's SHA-256 is recorded.  Kernel-level detail: `rocprofv3 --kernel-trace --stats -- python tools/gpu_adaptive.py --only cost`."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rtw_amd as R                      # noqa: E402
from rtw_amd import _capi                # noqa: E402
from rtw_amd.adaptive import DEFAULT_DARK_FLOOR, checkpoints  # noqa: E402
from gpu_progressive import HEADLINE, Frame, med, spread      # noqa: E402

N_CHUNKS = 250


def adaptive(f, acc, tol, gamma=1):
    """one fresh adaptive render of f's frame into f.buf -> (wall ms, info dict, stats)"""
    L = f.L
    f.check(L.rtw_accum_reset(acc, f.sp))
    f.stream.synchronize()
    A = _capi.Adaptive(tol, DEFAULT_DARK_FLOOR, 0, 0)
    P = _capi.make_params(f.width, f.height, f.spp, f.depth, 1, 0, gamma=gamma)
    t0 = time.perf_counter()
    f.check(L.rtw_render_adaptive_f32(f.scene, C.byref(f.cam), C.byref(P), C.byref(A), acc, C.c_void_p(f.buf.data_ptr()), f.sp))
    wall = (time.perf_counter() - t0) * 1e3
    info = _capi.AdaptiveInfo()
    f.check(L.rtw_accum_adaptive_info(acc, C.byref(info)))
    return wall, {k: getattr(info, k) for k, _ in info._fields_}, f.stats()


def accum_same_passes(f, acc, per_pass_stats):
    """rtw_render_accum_f32 over the adaptive render's pass structure, the last pass writing the image -> (wall ms, summed kernel ms)"""
    L = f.L
    f.check(L.rtw_accum_reset(acc, f.sp))
    f.stream.synchronize()
    cuts = [0] + checkpoints(N_CHUNKS) + [N_CHUNKS]
    kernel = 0.0
    t0 = time.perf_counter()
    for k, (b, e) in enumerate(zip(cuts[:-1], cuts[1:])):
        out = C.c_void_p(f.buf.data_ptr()) if k == len(cuts) - 2 else None
        f.check(L.rtw_render_accum_f32(f.scene, C.byref(f.cam), C.byref(f.P), b, e - b, acc, out, f.sp))
        if per_pass_stats:
            kernel += f.stats().kernel_ms
    f.stats()
    return (time.perf_counter() - t0) * 1e3, kernel


def tile_chunks(f, acc):
    n_tiles = ((f.height + 7) // 8) * ((f.width + 7) // 8)
    buf = np.zeros(n_tiles, np.int32)
    n = C.c_int32()
    f.check(f.L.rtw_accum_tile_chunks(acc, n_tiles, C.byref(n), buf.ctypes.data_as(C.POINTER(C.c_int32))))
    return buf


def linear_image(f):
    f.stream.synchronize()
    return f.buf.cpu().numpy().astype(np.float64)


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def measure_cost(L, a, res):
    f = Frame(L, **HEADLINE)
    acc = C.c_void_p()
    f.check(L.rtw_accum_create(0, f.width, f.height, C.byref(acc)))
    f.single()
    ref = f.hash()
    f.clear()
    _, info, st = adaptive(f, acc, 1e-300)
    if f.hash() != ref or info["tiles_at_cap"] != info["n_tiles"]:
        print("the adaptive frame at an unreachable tolerance DIFFERS from the one-shot render", file=sys.stderr)
        return False
    f.clear()
    accum_same_passes(f, acc, False)
    if f.hash() != ref:
        print("the progressive frame DIFFERS from the one-shot render", file=sys.stderr)
        return False
    single_t, ad_t, ad_k, ac_t, ac_k = [], [], [], [], []
    for _ in range(a.reps):
        single_t.append(f.single())
        w, _, st = adaptive(f, acc, 1e-300)
        ad_t.append(w); ad_k.append(st.kernel_ms)
        ac_t.append(accum_same_passes(f, acc, False)[0])
        ac_k.append(accum_same_passes(f, acc, True)[1])
    out = {"frame": "scene_random_spheres t_cam1 1920x1080 1000 spp (250 chunks of 4) depth 50 f32", "sha256": ref, "frames_identical": True,
           "passes": info["rounds"], "chunks_per_pass": checkpoints(N_CHUNKS)[0],
           "single_render": {"wall_ms_median": med([t[0] for t in single_t]), "wall_ms_min_max": spread([t[0] for t in single_t]),
                             "kernel_ms_median": med([t[1] for t in single_t])},
           "accum_same_passes": {"wall_ms_median": med(ac_t), "wall_ms_min_max": spread(ac_t), "kernel_ms_sum_median": med(ac_k)},
           "adaptive_unreachable_tolerance": {"wall_ms_median": med(ad_t), "wall_ms_min_max": spread(ad_t), "kernel_ms_sum_median": med(ad_k)}}
    out["adaptive_vs_accum_wall"] = round(med(ad_t) / med(ac_t), 4)
    out["adaptive_vs_accum_kernel"] = round(med(ad_k) / med(ac_k), 4)
    out["adaptive_vs_single_wall"] = round(med(ad_t) / med([t[0] for t in single_t]), 4)
    print("cost", json.dumps(out), flush=True)
    L.rtw_accum_free(acc)
    res["cost"] = out
    return True


def measure_gain(L, a, res):
    f = Frame(L, **HEADLINE)
    acc = C.c_void_p()
    f.check(L.rtw_accum_create(0, f.width, f.height, C.byref(acc)))
    # the yardstick: one uniform render of 4000 spp, linear
    y = Frame(L, HEADLINE["width"], 4000, HEADLINE["depth"])
    y.P = _capi.make_params(y.width, y.height, 4000, y.depth, 1, 0, gamma=0)
    y.single()
    yard = linear_image(y)
    out = {"yardstick": {"spp": 4000, "sha256": y.hash()}, "dark_floor": DEFAULT_DARK_FLOOR, "checkpoints": checkpoints(N_CHUNKS), "rows": []}
    f.P = _capi.make_params(f.width, f.height, f.spp, f.depth, 1, 0, gamma=0)
    f.single()
    ts = [f.single() for _ in range(a.reps)]
    uni = {"spp": 1000, "wall_ms_median": med([t[0] for t in ts]), "rmse_vs_4000spp": rmse(linear_image(f), yard), "sha256": f.hash()}
    out["uniform_1000spp"] = uni
    print("uniform", json.dumps(uni), flush=True)
    full = f.width * f.height * 1000
    for tol in a.tolerances:
        f.clear()
        walls = []
        for _ in range(a.reps):
            w, info, st = adaptive(f, acc, tol, gamma=0)
            walls.append(w)
        ct = tile_chunks(f, acc)
        cuts = [0] + checkpoints(N_CHUNKS)
        row = {"tolerance": tol, "samples": info["samples"], "samples_vs_uniform": round(info["samples"] / full, 4), "stats_samples": st.samples,
               "wall_ms_median": med(walls), "wall_ms_min_max": spread(walls), "wall_vs_uniform": round(med(walls) / uni["wall_ms_median"], 4),
               "kernel_ms_sum": round(st.kernel_ms, 3), "passes": info["rounds"],
               "active_tiles_per_pass": [int((ct > c).sum()) for c in cuts if (ct > c).any()],
               "tiles_converged": info["tiles_converged"], "tiles_at_cap": info["tiles_at_cap"],
               "rmse_vs_4000spp": rmse(linear_image(f), yard), "sha256": f.hash()}
        row["reaches_uniform_error"] = row["rmse_vs_4000spp"] <= uni["rmse_vs_4000spp"]
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    L.rtw_accum_free(acc)
    res["gain"] = out
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tolerances", default="0.1,0.05,0.03,0.02,0.01")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_frames.json"))
    ap.add_argument("--only", default="cost,gain")
    a = ap.parse_args()
    a.tolerances = [float(t) for t in a.tolerances.split(",")]
    import torch                         # torch's HIP runtime first: the frames live in torch buffers
    torch.cuda.init()
    L = _capi.lib()
    res = {"tool": "tools/gpu_adaptive.py", "reps": a.reps}
    ok = True
    if "cost" in a.only:
        ok &= measure_cost(L, a, res)
    if "gain" in a.only:
        ok &= measure_gain(L, a, res)
    if ok:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
