#!/usr/bin/env python3
"""The wide-aperture stage on one MI355X (include/rtw_hip.h rtw_wide_aperture_device_*): the measurements of DESIGN.md 7.27, written to
profiles/wide_aperture_frames.json.

    python tools/gpu_wide_aperture.py [--reps 50] [--warmup 5] [--out profiles/wide_aperture_frames.json]

The method is tools/gpu_defocus.py's: device events around `reps` back-to-back calls on one stream (a call returns before its
kernels end: the events end in a synchronise), after `warmup` calls of the same shape; the variants of a comparison alternate in the same
process and the median over 5 rounds is reported with the spread of the rounds.
  stage   the whole stage (six launches) at 1920 x 1080 and 480 x 270, Float32 and Float64, on scene_random_spheres through t_cam1's geometry
          (lookfrom (13, 2, 3) -> (0, 0, 0), vfov 20, focus 10), rendered through the pinhole at 1 spp with its real features, with lens radii chosen
          so that K -- the radius of the sky's circle of confusion -- is 8, 16 and 32 px, under max_radius 16 and under max_radius 32.  The
          yardstick of the same run, alternating with them: the defocus stage (two launches) at K = 8 under max_radius 8 -- the narrow gather
          is a part of the new stage, so the new stage cannot be cheaper.  The workspace is read back: the share of pixels with R > 8 (t = 1: the
          narrow gather's result is not used there) and with R <= 4, the small tiles by m, and the share of 16 x 16 tiles that lie wholly at
          t >= 1.  Next to them the trace kernel's own time (rtw_stats) for a 1-spp render through the LENS camera, which is what the stage replaces.
  split   the six launches one by one: a CHILD process runs the stage `split_reps` times per case under the library's measurement aid
          (RTW_ENABLE_TEST_AIDS=1 RTW_TEMPORAL_PROFILE=1: events around every launch, each call blocks), the parent takes the medians of the
          lines on its stderr.  These are single launches on an idle device, not back-to-back ones: they need not add up to `stage`.
          `narrow_skip_estimate_ms` is an ESTIMATE, not a measurement: the narrow gather's time scaled by the share of tiles wholly at t >= 1."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(1920, 1080), (480, 270)]
KS = [8.0, 16.0, 32.0]
RADII = [16, 32]
CAM = dict(lookfrom=(13, 2, 3), lookat=(0, 0, 0), vup=(0, 1, 0), vfov=20, aspect_ratio=16 / 9, focus_dist=10)
LAUNCHES = ("prepare", "gather", "wide_prepare", "reduce", "small_gather", "compose")


def frame(R, np, torch, T, W):
    """-> the pinhole camera, the scene, and the device image and features of its 1-spp render"""
    pin = R.default_camera(aperture=0, elem_type=T, **CAM)
    scene = R.scene_random_spheres(elem_type=T)
    image = np.ascontiguousarray(np.swapaxes(R.render(scene, pin, W, 1, seed=1, gamma=False, device=0), 0, 1))
    feat = np.ascontiguousarray(np.swapaxes(R.render_features(scene, pin, W, 1, seed=1, device=0)["raw"], 0, 1))
    return pin, scene, torch.from_numpy(image.ravel()).to("cuda:0"), torch.from_numpy(feat.ravel()).to("cuda:0")


def lens_radius_for(np, cam, W, K):
    return K * float(np.linalg.norm(np.asarray(cam.horizontal, np.float64))) / W


def child(a):
    import numpy as np
    import torch
    import rtw_amd as R
    torch.cuda.init()
    for T in (np.float32, np.float64):
        dt = torch.float64 if T is np.float64 else torch.float32
        for W, H in SHAPES:
            pin, _, image, feat = frame(R, np, torch, T, W)
            work = torch.zeros(max(R.wide_aperture_work_bytes(W, H, T, mr) for mr in RADII) // np.dtype(T).itemsize, dtype=dt, device="cuda:0")
            out = torch.zeros(W * H * 3, dtype=dt, device="cuda:0")
            for mr in RADII:
                for K in KS:
                    sys.stderr.write(f"[case] {K} {mr}\n")
                    sys.stderr.flush()
                    for _ in range(a.split_reps):
                        R.wide_aperture_into(out.data_ptr(), work.data_ptr(), image.data_ptr(), feat.data_ptr(), pin, W, H, elem_type=T, max_radius=mr,
                                             lens_radius=lens_radius_for(np, pin, W, K))
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--split-reps", type=int, default=21)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_aperture_frames.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    import numpy as np
    import torch                             # (torch's HIP runtime first: INTEGRATION.md section 5)
    import rtw_amd as R
    torch.cuda.init()
    if not torch.cuda.is_available():
        sys.exit("gpu_wide_aperture.py measures on a GPU: none found")

    def alternate(fns):
        """the variants of a comparison, round-robin, so that a drift of the machine meets all of them"""
        res = {k: [] for k in fns}
        for k, fn in fns.items():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                e1.synchronize()
                res[k].append(e0.elapsed_time(e1) / a.reps)
        return {k: {"ms": statistics.median(v), "min": min(v), "max": max(v)} for k, v in res.items()}

    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "rounds": a.rounds,
           "time": "device events around `reps` back-to-back calls on the null stream, per call; median (min, max) over the rounds",
           "split_time": "a child process under RTW_TEMPORAL_PROFILE: events around each single launch, the call blocks; median over split_reps calls",
           "stage": [], "split": []}
    shares = {}
    for T in (np.float32, np.float64):
        eb = np.dtype(T).itemsize
        dt = torch.float64 if T is np.float64 else torch.float32
        for W, H in SHAPES:
            pin, scene, image, feat = frame(R, np, torch, T, W)
            n, TH, TW = W * H, (H + 15) // 16, (W + 15) // 16
            work = torch.zeros(max(R.wide_aperture_work_bytes(W, H, T, mr) for mr in RADII) // eb, dtype=dt, device="cuda:0")
            nwork = torch.zeros(R.defocus_work_bytes(W, H, T) // eb, dtype=dt, device="cuda:0")
            res_img = torch.zeros(n * 3, dtype=dt, device="cuda:0")
            run = lambda K, mr: R.wide_aperture_into(res_img.data_ptr(), work.data_ptr(), image.data_ptr(), feat.data_ptr(), pin, W, H, elem_type=T, max_radius=mr,
                                                     lens_radius=lens_radius_for(np, pin, W, K))
            frames = {}
            for mr in RADII:
                s = 2 if mr <= 16 else 4
                h, w = (H + s - 1) // s, (W + s - 1) // s
                th, tw = (h + 15) // 16, (w + 15) // 16
                for K in KS:
                    run(K, mr)
                    torch.cuda.synchronize()
                    flat = work.cpu().numpy()
                    at = n * 4 + (TH * TW + 3) // 4 * 4                       # the wide CoC plane, behind the narrow stage's workspace
                    coc = flat[at:at + n * 4].reshape(W, H, 4)
                    Rw, ok = coc[..., 0], ~np.isnan(coc[..., 1])
                    pad = np.full((TW * 16, TH * 16), np.inf, T)              # (pixels outside the frame or not valid do not hold a tile back)
                    pad[:W, :H] = np.where(ok, Rw, np.inf)
                    whole = pad.reshape(TW, 16, TH, 16).min(axis=(1, 3)) >= 8
                    at_lo = at + n * 4 + (TH * TW + 3) // 4 * 4 + (n * 3 + 3) // 4 * 4 + (h * w * 3 + 3) // 4 * 4 + h * w * 4
                    tp = flat[at_lo:at_lo + th * tw].reshape(tw, th)
                    rn = np.array([[tp[max(0, b - 1):b + 2, max(0, c - 1):c + 2].max() for c in range(tp.shape[1])] for b in range(tp.shape[0])])
                    m = np.where(rn >= 0.5, np.ceil(rn.astype(T) + T(0.5)) - 1, 0).astype(np.int64)
                    frames[f"K{K:g}_max_radius{mr}"] = {"share_R_above_8": float((ok & (Rw > 8)).mean()), "share_R_up_to_4": float((ok & (Rw <= 4)).mean()),
                                                        "share_tiles_wholly_at_t1": float(whole.mean()), "small_tiles": int(tp.size), "small_tiles_by_m": [int((m == k).sum()) for k in range(9)]}
                    shares[(np.dtype(T).name.replace("float", "f"), W, H, K, mr)] = float(whole.mean())
            lens_ms = {}
            for K in KS:
                lens = R.default_camera(aperture=2 * lens_radius_for(np, pin, W, K), elem_type=T, **CAM)
                ms = []
                for _ in range(3):
                    R.render(scene, lens, W, 1, seed=1, gamma=False, device=0)
                    ms.append(R.last_stats()["kernel_ms"])
                lens_ms[f"K{K:g}"] = statistics.median(ms)
            fns = {"defocus_K8_max_radius8": lambda: R.defocus_into(res_img.data_ptr(), nwork.data_ptr(), image.data_ptr(), feat.data_ptr(), pin, W, H, elem_type=T, max_radius=8,
                                                                    lens_radius=lens_radius_for(np, pin, W, 8.0))}
            for mr in RADII:
                for K in KS:
                    fns[f"wide_K{K:g}_max_radius{mr}"] = lambda K=K, mr=mr: run(K, mr)
            res = alternate(fns)
            row = {"precision": np.dtype(T).name, "width": W, "height": H, **res, "frames": frames, "lens_render_1spp_kernel_ms": lens_ms}
            out["stage"].append(row)
            print(json.dumps(row), flush=True)
    # ---- the six launches one by one, in a child process under the measurement aid
    env = dict(os.environ, RTW_ENABLE_TEST_AIDS="1", RTW_TEMPORAL_PROFILE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--split-reps", str(a.split_reps)], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.exit(f"the child failed ({r.returncode}): {r.stderr[-2000:]}")
    case, rows = None, {}
    pat = r"\[rtw wide_aperture\] (f32|f64) (\d+)x(\d+) max_radius=(\d+) " + " ".join(k + r"_ms=([\d.]+)" for k in LAUNCHES)
    for line in r.stderr.splitlines():
        m = re.match(r"\[case\] ([\d.]+) (\d+)", line)
        if m:
            case = (float(m.group(1)), int(m.group(2)))
            continue
        m = re.match(pat, line)
        if m:
            rows.setdefault((m.group(1), int(m.group(2)), int(m.group(3)), case), []).append(tuple(float(m.group(k)) for k in range(5, 11)))
    for (prec, W, H, (K, mr)), v in rows.items():
        v = v[len(v) // 3:]                              # (the first third warms up)
        row = {"precision": prec, "width": W, "height": H, "K": K, "max_radius": mr, "calls": len(v)}
        for k, name in enumerate(LAUNCHES):
            row[name + "_ms"] = {"ms": statistics.median(x[k] for x in v), "min": min(x[k] for x in v), "max": max(x[k] for x in v)}
        row["dominant"] = max(LAUNCHES, key=lambda name: row[name + "_ms"]["ms"])
        share = shares.get((prec, W, H, K, mr))
        if share is not None:
            row["narrow_skip_estimate_ms"] = row["gather_ms"]["ms"] * share
        out["split"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
