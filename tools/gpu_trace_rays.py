#!/usr/bin/env python3
"""Radiance queries (include/rtw_hip.h rtw_trace_rays_device_*) on one MI355X: Msamples/s and kernel ms on scene_random_spheres (485
spheres), depth 16, Float32 and Float64.
usage: python tools/gpu_trace_rays.py [--reps 9] [--warmup 2] [--out profiles/trace_rays_frames.json]

Ray sets, all through t_cam1 (the headline camera), device-resident on one stream:
  primary_spp1 / primary_spp16    the 1920 x 1080 rays through the pixel centres, scanline order, 1 and 16 samples each
  permuted_spp1 / permuted_spp16  the same rays in a random permutation
  probe_4096x256                  4 096 of those rays (every 506th) with 256 samples each: few rays, many samples
Yardstick of the primary sets: rtw_render_device_* of the same frame, spp and depth (plain scan, and with RTW_FLAG_GROUP_CULL, the
benchmark's mode), in samples per second -- the same scans and scatters behind an item scheduler that deals (pixel, chunk) items to lanes;
the trace kernel's sources and ISA are the parent commit's (profiles/trace_rays_isa_compare.txt).  Query and renders are timed ALTERNATELY
in the same loop.
Per case: the kernel's HIP-event time from rtw_stats() (kernel_ms) of --reps calls after --warmup: the median and the spread (min, max);
segments per sample from the same record.  The matrix-pipe and the RTW_FLAG_SCAN_VALU call of a set must give identical bytes."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch                             # noqa: E402  (torch's HIP runtime first: INTEGRATION.md section 5)
import rtw_amd as R                      # noqa: E402
from rtw_amd import _capi                # noqa: E402
from gpu_rays import primary_rays, W, H  # noqa: E402

DEPTH = 16


def run_precision(T, reps, warmup):
    L = _capi.lib()
    f64 = np.dtype(T) == np.float64
    sfx = "f64" if f64 else "f32"
    R.reseed()                           # reseed!(): the same scene in every case (485 spheres in Float32)
    scene = R.scene_random_spheres(elem_type=T)
    cam_obj = R.t_cam1(elem_type=T)
    dr = R.DeviceRenderer(scene, cam_obj, 0)
    tdt = torch.float64 if f64 else torch.float32
    stream = torch.cuda.Stream()
    d_img = torch.empty(W * H * 3, dtype=tdt, device="cuda:0")

    def renderer(spp, cull):
        def go():
            dr.render_into(d_img.data_ptr(), W, spp, depth=DEPTH, seed=1, stream=stream.cuda_stream, group_cull=cull)
            return dr.stats()
        return go

    def tracer(d_rays, n, d_out, spp, flags):
        def go():
            dr.trace_rays_into(d_rays.data_ptr(), n, d_out.data_ptr(), spp=spp, max_depth=DEPTH, seed=1, flags=flags, stream=stream.cuda_stream)
            return dr.stats()
        return go

    def timed(fns):
        """the functions called alternately: warmup rounds, then reps rounds -> per function (last stats, median, min, max)"""
        for _ in range(warmup):
            for fn in fns:
                fn()
        sts = [[] for _ in fns]
        for _ in range(reps):
            for k, fn in enumerate(fns):
                sts[k].append(fn())
        out = []
        for s in sts:
            ms = [x["kernel_ms"] for x in s]
            out.append((s[-1], statistics.median(ms), min(ms), max(ms)))
        return out

    def entry(st, med, lo, hi):
        return {"kernel_ms_median": round(med, 5), "kernel_ms_min_max": [round(lo, 5), round(hi, 5)], "msamples_s": round(st["samples"] / med * 1e-3, 1),
                "segments_per_sample": round(st["segments"] / st["samples"], 4), "grid_blocks": int(st["grid_blocks"])}

    res = {}
    primary = primary_rays(cam_obj, T, False)
    rng = np.random.default_rng(5)
    sets = {"primary": primary, "permuted": primary[rng.permutation(W * H)], "probe": primary[::506][:4096]}
    for name, spp in (("primary", 1), ("permuted", 1), ("primary", 16), ("permuted", 16), ("probe", 256)):
        rays = sets[name]
        n = rays.shape[0]
        d_rays = torch.from_numpy(np.ascontiguousarray(rays)).to("cuda:0")
        d_out = torch.empty(n * 3, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        fns = [tracer(d_rays, n, d_out, spp, 0), tracer(d_rays, n, d_out, spp, _capi.FLAG_SCAN_VALU)]
        fns[0]()
        torch.cuda.synchronize()
        ref = d_out.cpu().numpy().copy()
        fns[1]()
        torch.cuda.synchronize()
        same = d_out.cpu().numpy().tobytes() == ref.tobytes()
        r = {"rays": n, "spp": spp, "depth": DEPTH, "dtype": np.dtype(T).name, "spheres": dr.n_spheres, "mean_radiance": [round(float(x), 6) for x in ref.reshape(-1, 3).mean(axis=0)]}
        if name == "probe":
            (st_m, *m), (st_v, *v) = timed(fns)
        else:
            (st_m, *m), (st_v, *v), (st_r, *rr), (st_c, *rc) = timed(fns + [renderer(spp, False), renderer(spp, True)])
            assert st_r["samples"] == W * H * spp == st_m["samples"]
            r["render_plain"] = entry(st_r, *rr)
            r["render_group_cull"] = entry(st_c, *rc)
            r["query_rate_over_render_plain"] = round(rr[0] / m[0], 4)
            r["query_rate_over_render_group_cull"] = round(rc[0] / m[0], 4)
        r["matrix"] = entry(st_m, *m)
        r["valu"] = entry(st_v, *v)
        r["valu_bytes_identical"] = bool(same)
        key = f"{sfx}_{name}_{n}x{spp}" if name == "probe" else f"{sfx}_{name}_spp{spp}"
        res[key] = r
        print(key, json.dumps(r), flush=True)
        del d_rays, d_out
    dr.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_rays_frames.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("no GPU: nothing is measured here", file=sys.stderr)
        return 1
    torch.cuda.init()
    res = {"tool": "tools/gpu_trace_rays.py", "reps": a.reps, "warmup": a.warmup, "width": W, "height": H,
           "time": "rtw_stats().kernel_ms (HIP events around the kernel); the two calls of a ray set and the two renders alternate in one loop",
           "render_library": "this tree's librtw_hip.so, not a build of the parent commit: the trace kernel's instances are the parent's instruction for instruction (profiles/trace_rays_isa_compare.txt)", "cases": {}}
    for T in (np.float32, np.float64):
        res["cases"].update(run_precision(T, a.reps, a.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0 if all(r["valu_bytes_identical"] for r in res["cases"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
