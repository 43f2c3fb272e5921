#!/usr/bin/env python3
"""Ray queries (include/rtw_hip.h rtw_cast_rays_device_*) on one MI355X: Mrays/s and kernel ms on scene_random_spheres (485 spheres), with
records, matrix pipe against RTW_FLAG_SCAN_VALU, Float32 and Float64.
usage: python tools/gpu_rays.py [--reps 15] [--warmup 3] [--out profiles/rays_frames.json]

Ray sets, all through t_cam1 (the headline camera), device-resident on one stream:
  primary           the 1920 x 1080 primary rays through the pixel centres, scanline order (a wave = 64 neighbours of one row)
  primary_tiles     the same rays in the feature kernel's order: 8 x 8 tiles, a wave = one tile (not asked for by a caller, shown for comparison)
  permuted          the same rays in a random permutation
  bounce            one ray per hit of `primary`: from the hit point into a random direction
  n64, n4096, n65536   the first n rays of `primary`: the small-launch regime
Yardstick of `primary`: the feature pass (rtw_render_features_device_*) over the same frame with ONE chunk of one sample -- the same scan
over the same number of primary rays plus an RNG, against 68 (Float32) / 132 (Float64) bytes of traffic per ray here.  The two are timed
ALTERNATELY in the same loop.
Per case: the kernel's HIP-event time from rtw_stats() (kernel_ms) of --reps calls after --warmup: the median and the spread (min, max).
The matrix-pipe and the VALU call of a set must give identical bytes."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                             # noqa: E402  (torch's HIP runtime first: INTEGRATION.md section 5)
import rtw_amd as R                      # noqa: E402
from rtw_amd import _capi                # noqa: E402

W, H = 1920, 1080


def primary_rays(cam, T, tiles):
    o, llc, hor, ver = (np.asarray(getattr(cam, k), np.float64) for k in ("origin", "lower_left_corner", "horizontal", "vertical"))
    if tiles:            # tiles numbered column-major, lane = (i mod 8) + 8 (j mod 8): the feature kernel's decomposition
        tj, ti, lj, li = np.meshgrid(np.arange(W // 8), np.arange(H // 8), np.arange(8), np.arange(8), indexing="ij")
        i, j = (ti * 8 + li).ravel(), (tj * 8 + lj).ravel()
    else:
        i, j = (a.ravel() for a in np.meshgrid(np.arange(H), np.arange(W), indexing="ij"))
    u, v = ((j + 0.5) / W)[:, None], ((H - 1 - i + 0.5) / H)[:, None]
    d = llc + u * hor + v * ver - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((i.size, 8), T)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = o, d, np.inf, j * H + i
    return rays


def run_precision(T, reps, warmup):
    L = _capi.lib()
    f64 = np.dtype(T) == np.float64
    sfx = "f64" if f64 else "f32"
    R.reseed()                           # reseed!(): the same scene in every case (485 spheres in Float32)
    flat = R.flatten_scene(R.scene_random_spheres(elem_type=T), T)
    S, keep = _capi.make_scene(flat, T)
    cam_obj = R.t_cam1(elem_type=T)
    cam = _capi.make_camera(cam_obj, T)
    handle = C.c_void_p()
    _capi.check(getattr(L, "rtw_scene_upload_" + sfx)(C.byref(S), 0, C.byref(handle)))
    tdt = torch.float64 if f64 else torch.float32
    stream = torch.cuda.Stream()
    cast = getattr(L, "rtw_cast_rays_device_" + sfx)
    f_feat = getattr(L, "rtw_render_features_device_" + sfx)
    d_feat = torch.empty(W * H * 8, dtype=tdt, device="cuda:0")

    def stats():
        st = _capi.Stats()
        _capi.check(L.rtw_stats(C.byref(st)))
        return st

    def features():
        P = _capi.make_params(W, H, 1, 16, 1, 1)
        _capi.check(f_feat(handle, C.byref(cam), C.byref(P), 0, 1, C.c_void_p(d_feat.data_ptr()), C.c_void_p(stream.cuda_stream)))
        return stats()

    def caster(d_rays, n, d_idx, d_rec, flags):
        P = R.make_rays_params(flags=flags)

        def go():
            _capi.check(cast(handle, C.c_void_p(d_rays.data_ptr()), n, C.byref(P), C.c_void_p(d_idx.data_ptr()), C.c_void_p(d_rec.data_ptr()), C.c_void_p(stream.cuda_stream)))
            return stats()
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
            ms = [x.kernel_ms for x in s]
            out.append((s[-1], statistics.median(ms), min(ms), max(ms)))
        return out

    def entry(st, med, lo, hi, n):
        return {"kernel_ms_median": round(med, 5), "kernel_ms_min_max": [round(lo, 5), round(hi, 5)], "mrays_s": round(n / med * 1e-3, 1), "grid_blocks": int(st.grid_blocks)}

    res = {}
    sets = {"primary": primary_rays(cam_obj, T, False), "primary_tiles": primary_rays(cam_obj, T, True)}
    rng = np.random.default_rng(5)
    sets["permuted"] = sets["primary"][rng.permutation(W * H)]
    hit_rec = None
    for name in ("primary", "primary_tiles", "permuted", "bounce", "n64", "n4096", "n65536"):
        if name == "bounce":
            idx, rec = hit_rec
            hit = idx >= 0
            d = rng.normal(size=(int(hit.sum()), 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            rays = np.zeros((d.shape[0], 8), T)
            rays[:, 0:3], rays[:, 3:6], rays[:, 6] = rec[hit, 1:4], d, np.inf
        elif name.startswith("n"):
            rays = sets["primary"][:int(name[1:])]
        else:
            rays = sets[name]
        n = rays.shape[0]
        d_rays = torch.from_numpy(np.ascontiguousarray(rays)).to("cuda:0")
        d_idx = torch.empty(n, dtype=torch.int32, device="cuda:0")
        d_rec = torch.empty(n * 8, dtype=tdt, device="cuda:0")
        torch.cuda.synchronize()
        fns = [caster(d_rays, n, d_idx, d_rec, 0), caster(d_rays, n, d_idx, d_rec, _capi.FLAG_SCAN_VALU)]
        # (bytes first, one call each: the VALU call last leaves its words in the buffers while the matrix pipe's are compared)
        fns[0]()
        torch.cuda.synchronize()
        ref = (d_idx.cpu().numpy().copy(), d_rec.cpu().numpy().copy())
        fns[1]()
        torch.cuda.synchronize()
        same = d_idx.cpu().numpy().tobytes() == ref[0].tobytes() and d_rec.cpu().numpy().tobytes() == ref[1].tobytes()
        if name == "primary":
            hit_rec = (ref[0], ref[1].reshape(-1, 8))
            (st_m, *m), (st_v, *v), (st_f, *f) = timed(fns + [features])
            assert st_f.segments == W * H and st_m.segments == n
        else:
            (st_m, *m), (st_v, *v) = timed(fns)
        r = {"rays": n, "dtype": np.dtype(T).name, "spheres": int(flat["n"]), "hits": round(float((ref[0] >= 0).mean()), 4),
             "matrix": entry(st_m, *m, n), "valu": entry(st_v, *v, n), "valu_bytes_identical": bool(same),
             "matrix_over_valu": round(m[0] / v[0], 4)}
        if name == "primary":
            r["feature_pass_one_chunk"] = entry(st_f, *f, W * H)
            r["rays_over_feature_pass"] = round(m[0] / f[0], 4)
        res[f"{sfx}_{name}"] = r
        print(f"{sfx}_{name}", json.dumps(r), flush=True)
        del d_rays, d_idx, d_rec
    L.rtw_scene_free(handle)
    del keep
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rays_frames.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("no GPU: nothing is measured here", file=sys.stderr)
        return 1
    torch.cuda.init()
    res = {"tool": "tools/gpu_rays.py", "reps": a.reps, "warmup": a.warmup, "width": W, "height": H,
           "time": "rtw_stats().kernel_ms (HIP events around the kernel); the calls of a ray set, and the feature pass, alternate in one loop", "cases": {}}
    for T in (np.float32, np.float64):
        res["cases"].update(run_precision(T, a.reps, a.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0 if all(r["valu_bytes_identical"] for r in res["cases"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
