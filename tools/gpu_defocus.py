#!/usr/bin/env python3
"""The defocus stage on one MI355X (include/rtw_hip.h rtw_defocus_device_*): the measurements of DESIGN.md 7.25, written to
profiles/defocus_frames.json.

    python tools/gpu_defocus.py [--reps 50] [--warmup 5] [--out profiles/defocus_frames.json]

The method is tools/gpu_motion_blur.py's: device events around `reps` back-to-back calls on one stream (a call returns before its kernels end:
the events end in a synchronise), after `warmup` calls of the same shape; the variants of a comparison alternate in the same process and the
median over 5 rounds is reported with the spread of the rounds.
  stage   the whole stage (two launches) at 1920 x 1080 and 480 x 270, Float32 and Float64, on scene_random_spheres through t_cam1's geometry
          (lookfrom (13, 2, 3) -> (0, 0, 0), vfov 20, focus 10), rendered through the pinhole at 1 spp with its real features, with lens radii chosen
          so that K -- the radius of the sky's circle of confusion, which is what most neighbourhoods' RN is -- is 2, 4 and 8 px.  The workspace is
          read back: the share of tiles that take the early-out, the median RN, the tiles by m.  `defocus_K2_max_radius2` is K = 2 under
          max_radius 2 -- radii above 2 px are clamped, the launch's LDS window is 20 columns, not 32: what the allocation by max_radius costs
          at small m.  Yardsticks of the same run: the 15-tap motion blur of the same frame under a motion plane that moves every surface by
          8 px (every tile filters), and the trace kernel's own time (rtw_stats) for a 1-spp render through the LENS camera, which is what the
          stage replaces.
  split   the two launches one by one: a CHILD process runs the stage `split_reps` times per case under the library's measurement aid
          (RTW_ENABLE_TEST_AIDS=1 RTW_TEMPORAL_PROFILE=1: events around every launch, each call blocks), the parent takes the medians of the
          lines on its stderr.  These are single launches on an idle device, not back-to-back ones: they need not add up to `stage`."""
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
KS = [2.0, 4.0, 8.0]
CAM = dict(lookfrom=(13, 2, 3), lookat=(0, 0, 0), vup=(0, 1, 0), vfov=20, aspect_ratio=16 / 9, focus_dist=10)


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
            work = torch.zeros(R.defocus_work_bytes(W, H, T) // np.dtype(T).itemsize, dtype=dt, device="cuda:0")
            out = torch.zeros(W * H * 3, dtype=dt, device="cuda:0")
            for K in KS:
                sys.stderr.write(f"[case] {K}\n")
                sys.stderr.flush()
                for _ in range(a.split_reps):
                    R.defocus_into(out.data_ptr(), work.data_ptr(), image.data_ptr(), feat.data_ptr(), pin, W, H, elem_type=T, lens_radius=lens_radius_for(np, pin, W, K))
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--split-reps", type=int, default=21)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "defocus_frames.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    import numpy as np
    import torch                             # (torch's HIP runtime first: INTEGRATION.md section 5)
    import rtw_amd as R
    torch.cuda.init()
    if not torch.cuda.is_available():
        sys.exit("gpu_defocus.py measures on a GPU: none found")

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

    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "rounds": a.rounds, "max_radius": 8,
           "time": "device events around `reps` back-to-back calls on the null stream, per call; median (min, max) over the rounds",
           "split_time": "a child process under RTW_TEMPORAL_PROFILE: events around each single launch, the call blocks; median over split_reps calls",
           "stage": [], "split": []}
    for T in (np.float32, np.float64):
        eb = np.dtype(T).itemsize
        dt = torch.float64 if T is np.float64 else torch.float32
        for W, H in SHAPES:
            pin, scene, image, feat = frame(R, np, torch, T, W)
            n = W * H
            work = torch.zeros(R.defocus_work_bytes(W, H, T) // eb, dtype=dt, device="cuda:0")
            bwork = torch.zeros(R.motion_blur_work_bytes(W, H, T) // eb, dtype=dt, device="cuda:0")
            res_img = torch.zeros(n * 3, dtype=dt, device="cuda:0")
            px = float(np.linalg.norm(np.asarray(pin.horizontal, np.float64))) / W          # one pixel on the focus plane
            moving = np.zeros((n, 4), T)
            moving[:, 0:3] = 8.0 * px * np.asarray(pin.u, np.float64)
            motion = torch.from_numpy(moving.ravel()).to("cuda:0")
            run = lambda K, mr=8: R.defocus_into(res_img.data_ptr(), work.data_ptr(), image.data_ptr(), feat.data_ptr(), pin, W, H, elem_type=T, max_radius=mr,
                                                 lens_radius=lens_radius_for(np, pin, W, K))
            tiles = {}
            for K in KS:
                run(K)
                torch.cuda.synchronize()
                tp = work.cpu().numpy()[n * 4:][:((H + 15) // 16) * ((W + 15) // 16)].reshape((W + 15) // 16, (H + 15) // 16)
                rn = np.array([[tp[max(0, b - 1):b + 2, max(0, c - 1):c + 2].max() for c in range(tp.shape[1])] for b in range(tp.shape[0])])
                m = np.where(rn >= 0.5, np.ceil(rn.astype(T) + T(0.5)) - 1, 0).astype(np.int64)
                tiles[str(K)] = {"tiles": int(tp.size), "tiles_early_out": int((~(rn >= 0.5)).sum()), "median_RN": float(np.median(rn)), "largest_RN": float(rn.max()),
                                 "tiles_by_m": [int((m[rn >= 0.5] == k).sum()) for k in range(9)], "mean_taps_per_pixel_of_filtering_tiles": float(((2 * m[rn >= 0.5] + 1) ** 2).mean())}
                lens = R.default_camera(aperture=2 * lens_radius_for(np, pin, W, K), elem_type=T, **CAM)
                ms = []
                for _ in range(3):
                    R.render(scene, lens, W, 1, seed=1, gamma=False, device=0)
                    ms.append(R.last_stats()["kernel_ms"])
                tiles[str(K)]["lens_render_1spp_kernel_ms"] = statistics.median(ms)
            fns = {f"defocus_K{K:g}": (lambda K=K: run(K)) for K in KS}
            fns["defocus_K2_max_radius2"] = lambda: run(2.0, 2)             # the same aperture under a window a quarter the size: 20 columns of LDS, not 32
            fns["motion_blur_15_taps"] = lambda: R.motion_blur_into(res_img.data_ptr(), bwork.data_ptr(), image.data_ptr(), feat.data_ptr(), motion.data_ptr(), pin, pin, W, H, elem_type=T)
            res = alternate(fns)
            row = {"precision": np.dtype(T).name, "width": W, "height": H, **res, "frames": tiles}
            out["stage"].append(row)
            print(json.dumps(row), flush=True)
    # ---- the two launches one by one, in a child process under the measurement aid
    env = dict(os.environ, RTW_ENABLE_TEST_AIDS="1", RTW_TEMPORAL_PROFILE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--split-reps", str(a.split_reps)], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.exit(f"the child failed ({r.returncode}): {r.stderr[-2000:]}")
    case, rows = None, {}
    for line in r.stderr.splitlines():
        m = re.match(r"\[case\] ([\d.]+)", line)
        if m:
            case = m.group(1)
            continue
        m = re.match(r"\[rtw defocus\] (f32|f64) (\d+)x(\d+) max_radius=\d+ prepare_ms=([\d.]+) gather_ms=([\d.]+)", line)
        if m:
            rows.setdefault((m.group(1), int(m.group(2)), int(m.group(3)), case), []).append(tuple(float(m.group(k)) for k in (4, 5)))
    for (prec, W, H, case), v in rows.items():
        v = v[len(v) // 3:]                              # (the first third warms up)
        row = {"precision": prec, "width": W, "height": H, "K": float(case), "calls": len(v)}
        for k, name in enumerate(("prepare_and_tile_max_ms", "gather_ms")):
            row[name] = {"ms": statistics.median(x[k] for x in v), "min": min(x[k] for x in v), "max": max(x[k] for x in v)}
        out["split"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
