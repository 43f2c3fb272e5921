#!/usr/bin/env python3
"""The motion-blur stage on one MI355X (include/rtw_hip.h rtw_velocity_blur_device_*): the measurements of DESIGN.md 7.24, written to
profiles/motion_blur_frames.json.

    python tools/gpu_motion_blur.py [--reps 100] [--warmup 10] [--out profiles/motion_blur_frames.json]

The method is tools/gpu_animation.py's: device events around `reps` back-to-back calls on one stream (a call returns before its kernels end:
the events end in a synchronise), after `warmup` calls of the same shape; the variants of a comparison alternate in the same process and the
median over 5 rounds is reported with the spread of the rounds.
  stage   the whole stage (three launches) at 1920 x 1080 and 480 x 270, Float32 and Float64, on two synthetic frames: `all` -- a wall at depth
          5 that moved about 8 px, every tile filters -- and `none` -- a zero plane and one camera, every tile passes through (the neighbour plane
          is read back and says how many tiles did filter).  Yardsticks of the same run: the plain temporal step, and one a-trous level
          (the denoiser with 2 levels minus the denoiser with 1).  hbm_share: the compulsory traffic -- image in, blur plane out and in,
          image out: 14 elements per pixel -- over the stage's time, as a share of 8 TB/s.
  split   the three launches one by one: a CHILD process runs the stage `split_reps` times per shape under the library's measurement aid
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
HBM_BYTES_PER_S = 8.0e12


def frames(R, np, torch, T, W, H):
    """-> cameras and device buffers of the two synthetic frames"""
    dt = torch.float64 if T is np.float64 else torch.float32
    cam = R.default_camera(lookfrom=(0, 0, 0), lookat=(0, 0, -1), vfov=60, aspect_ratio=W / H, aperture=0, focus_dist=1, elem_type=T)
    rng = np.random.default_rng(3)
    image = torch.from_numpy(rng.uniform(0, 1, W * H * 3).astype(T)).to("cuda:0")
    feat = np.zeros((W * H, 8), T)
    feat[:, 0:3], feat[:, 5], feat[:, 6], feat[:, 7] = 0.5, 1.0, 5.0, 1.0
    feat = torch.from_numpy(feat.ravel()).to("cuda:0")
    px = float(np.linalg.norm(np.asarray(cam.horizontal, np.float64))) / W * 5.0          # one pixel at depth 5 (focus_dist 1)
    moving = np.zeros((W * H, 4), T)
    moving[:, 0] = 8.0 * px
    return cam, image, feat, {"all": torch.from_numpy(moving.ravel()).to("cuda:0"), "none": torch.zeros(W * H * 4, dtype=dt, device="cuda:0")}, dt


def child(a):
    import numpy as np
    import torch
    import rtw_amd as R
    torch.cuda.init()
    for T in (np.float32, np.float64):
        for W, H in SHAPES:
            cam, image, feat, motion, dt = frames(R, np, torch, T, W, H)
            work = torch.zeros(R.motion_blur_work_bytes(W, H, T) // np.dtype(T).itemsize, dtype=dt, device="cuda:0")
            out = torch.zeros(W * H * 3, dtype=dt, device="cuda:0")
            for case in ("all", "none"):
                sys.stderr.write(f"[case] {case}\n")
                sys.stderr.flush()
                for _ in range(a.split_reps):
                    R.motion_blur_into(out.data_ptr(), work.data_ptr(), image.data_ptr(), feat.data_ptr(), motion[case].data_ptr(), cam, cam, W, H, elem_type=T)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--split-reps", type=int, default=30)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_blur_frames.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    import numpy as np
    import torch                             # (torch's HIP runtime first: INTEGRATION.md section 5)
    import rtw_amd as R
    torch.cuda.init()
    if not torch.cuda.is_available():
        sys.exit("gpu_motion_blur.py measures on a GPU: none found")

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

    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "rounds": a.rounds, "taps": 15, "shutter": 1.0,
           "time": "device events around `reps` back-to-back calls on the null stream, per call; median (min, max) over the rounds",
           "split_time": "a child process under RTW_TEMPORAL_PROFILE: events around each single launch, the call blocks; median over split_reps calls",
           "stage": [], "split": []}
    for T in (np.float32, np.float64):
        eb = np.dtype(T).itemsize
        for W, H in SHAPES:
            cam, image, feat, motion, dt = frames(R, np, torch, T, W, H)
            n = W * H
            work = torch.zeros(R.motion_blur_work_bytes(W, H, T) // eb, dtype=dt, device="cuda:0")
            dwork = torch.zeros(R.denoise_work_bytes(W, H, T) // eb, dtype=dt, device="cuda:0")
            res_img = torch.zeros(n * 3, dtype=dt, device="cuda:0")
            st = [torch.zeros(R.temporal_state_bytes(W, H, T) // eb, dtype=dt, device="cuda:0") for _ in range(2)]
            R.temporal_step_into(res_img.data_ptr(), st[0].data_ptr(), image.data_ptr(), feat.data_ptr(), cam, W, H, elem_type=T)
            blur = lambda case: R.motion_blur_into(res_img.data_ptr(), work.data_ptr(), image.data_ptr(), feat.data_ptr(), motion[case].data_ptr(), cam, cam, W, H, elem_type=T)
            tiles = {}
            for case in ("all", "none"):
                blur(case)
                torch.cuda.synchronize()
                nb = work.cpu().numpy()[n * 4:].reshape(2, -1, 4)[1]
                tiles[case] = {"tiles": int(nb.shape[0]), "tiles_that_filter": int((nb[:, 2] >= 0.5).sum()), "largest_half_extent_px": float(nb[:, 2].max())}
            res = alternate({"blur_all": lambda: blur("all"), "blur_none": lambda: blur("none"),
                             "temporal_step": lambda: R.temporal_step_into(res_img.data_ptr(), st[1].data_ptr(), image.data_ptr(), feat.data_ptr(), cam, W, H,
                                                                           d_state_prev_ptr=st[0].data_ptr(), cam_prev=cam, elem_type=T),
                             "denoise_1_level": lambda: R.denoise_into(res_img.data_ptr(), image.data_ptr(), feat.data_ptr(), dwork.data_ptr(), W, H, elem_type=T, levels=1),
                             "denoise_2_levels": lambda: R.denoise_into(res_img.data_ptr(), image.data_ptr(), feat.data_ptr(), dwork.data_ptr(), W, H, elem_type=T, levels=2)})
            compulsory = n * 14 * eb
            row = {"precision": np.dtype(T).name, "width": W, "height": H, **res, "frames": tiles,
                   "one_atrous_level_ms": res["denoise_2_levels"]["ms"] - res["denoise_1_level"]["ms"], "compulsory_bytes": compulsory,
                   "hbm_share_all": compulsory / (res["blur_all"]["ms"] * 1e-3) / HBM_BYTES_PER_S, "hbm_share_none": compulsory / (res["blur_none"]["ms"] * 1e-3) / HBM_BYTES_PER_S}
            out["stage"].append(row)
            print(json.dumps(row), flush=True)
    # ---- the three launches one by one, in a child process under the measurement aid
    env = dict(os.environ, RTW_ENABLE_TEST_AIDS="1", RTW_TEMPORAL_PROFILE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--split-reps", str(a.split_reps)], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.exit(f"the child failed ({r.returncode}): {r.stderr[-2000:]}")
    case, rows = None, {}
    for line in r.stderr.splitlines():
        m = re.match(r"\[case\] (\w+)", line)
        if m:
            case = m.group(1)
            continue
        m = re.match(r"\[rtw motion blur\] (f32|f64) (\d+)x(\d+) taps=\d+ velocity_ms=([\d.]+) neighbour_ms=([\d.]+) gather_ms=([\d.]+)", line)
        if m:
            rows.setdefault((m.group(1), int(m.group(2)), int(m.group(3)), case), []).append(tuple(float(m.group(k)) for k in (4, 5, 6)))
    for (prec, W, H, case), v in rows.items():
        v = v[len(v) // 3:]                              # (the first third warms up)
        row = {"precision": prec, "width": W, "height": H, "frame": case, "calls": len(v)}
        for k, name in enumerate(("velocity_and_tile_max_ms", "neighbour_max_ms", "gather_ms")):
            row[name] = {"ms": statistics.median(x[k] for x in v), "min": min(x[k] for x in v), "max": max(x[k] for x in v)}
        out["split"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
