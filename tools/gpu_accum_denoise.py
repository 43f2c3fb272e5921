#!/usr/bin/env python3
"""An adaptive accumulator as the denoiser's input on one MI355X (include/rtw_hip.h rtw_accum_features_f32, rtw_accum_noise_f32,
rtw_guided_filter_device_f32), kernel by kernel: the measurements of DESIGN.md 7.11.
usage: python tools/gpu_accum_denoise.py [--width 1920] [--spp 64] [--tolerance 0.05] [--out profiles/accum_denoise_frames.json]

The frame: scene_random_spheres through t_cam1 at --width (1920 x 1080), Float32, ONE adaptive render of at most --spp samples.  Then, in
the same process, 2 warm-ups and 7 timed rounds of: the tile-prefix feature pass (rtw_stats().kernel_ms), the noise map (HIP events of
the caller's stream around the call), the guided filter and the plain filter one after the other (levels = 5; HIP events around every
kernel, recorded by the library under the measurement aids RTW_ENABLE_TEST_AIDS=1 RTW_DENOISE_PROFILE=1, one line per kernel on stderr).
Per kernel the median of the 7 with min and max, and the time its compulsory HBM bytes would take at 6.3 TB/s:
  feature pass   32 B per pixel out (the tile counts are 4 B per 64 pixels)
  noise map      64 B per pixel in (the words), 4 B out
  prepare        12 + 32 B in (+ 4 B of map, guided), 3 planes of 16 B out
  level          E and G records in (32 B; guided: + the A slot that holds the variance, 16 B), colour out 16 B; the last level: the albedo in
                 (16 B, unless guided read it already) and the image out, 12 B"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3
WARMUP, REPS, LEVELS = 2, 7, 5
LINE = re.compile(r"^\[rtw denoise( guided)?\] f32 \d+x\d+ (prepare|level|total)(?: step=(\d+) final=(\d))?(?: levels=\d+)? ms=([0-9.]+)$")


def child(a):
    import numpy as np
    import torch                             # (torch's HIP runtime first: INTEGRATION.md section 5)
    import rtw_amd as R
    torch.cuda.init()
    T = np.float32
    R.reseed()
    scene, cam = R.scene_random_spheres(elem_type=T), R.t_cam1(elem_type=T)
    with R.AdaptiveRenderer(scene, cam, a.width, a.spp, device=0) as ar:
        info = ar.run(a.tolerance)
        st = ar.stats()
        W, H = ar.width, ar.height
        n = W * H
        d_img, d_out = (torch.empty(n * 3, dtype=torch.float32, device="cuda:0") for _ in range(2))
        d_feat = torch.empty(n * 8, dtype=torch.float32, device="cuda:0")
        d_noise = torch.empty(n, dtype=torch.float32, device="cuda:0")
        d_work = torch.empty(R.denoise_work_bytes(W, H, T) // 4, dtype=torch.float32, device="cuda:0")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        ar.resolve_into(d_img.data_ptr(), gamma=False, stream=stream.cuda_stream)
        feat_ms, noise_ms = [], []
        for _ in range(WARMUP + REPS):
            ar.features_into(d_feat.data_ptr(), stream=stream.cuda_stream)
            feat_ms.append(ar.stats()["kernel_ms"])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ar.noise_into(d_noise.data_ptr(), stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            noise_ms.append(e0.elapsed_time(e1))
            # guided and plain alternate: the same process, the same buffers, one after the other
            R.denoise_guided_into(d_out.data_ptr(), d_img.data_ptr(), d_feat.data_ptr(), d_noise.data_ptr(), d_work.data_ptr(), W, H, elem_type=T,
                                  stream=stream.cuda_stream, levels=LEVELS)
            R.denoise_into(d_out.data_ptr(), d_img.data_ptr(), d_feat.data_ptr(), d_work.data_ptr(), W, H, elem_type=T, stream=stream.cuda_stream, levels=LEVELS)
        stream.synchronize()
        ct = ar.tile_chunks()
    print(json.dumps({"width": W, "height": H, "spp": a.spp, "tolerance": a.tolerance, "adaptive_render_kernel_ms": round(st["kernel_ms"], 4),
                      "samples_share": round(info["samples"] / (n * a.spp), 4), "tiles": int(ct.size), "chunks_held_min_max": [int(ct.min()), int(ct.max())],
                      "chunks_held_mean": round(float(ct.mean()), 3), "feature_ms": [round(x, 5) for x in feat_ms[WARMUP:]],
                      "noise_ms": [round(x, 5) for x in noise_ms[WARMUP:]]}))
    return 0


def med(xs):
    return {"ms_median": round(statistics.median(xs), 5), "ms_min_max": [round(min(xs), 5), round(max(xs), 5)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--tolerance", type=float, default=0.05)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_denoise_frames.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    env = dict(os.environ, RTW_ENABLE_TEST_AIDS="1", RTW_DENOISE_PROFILE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--width", str(a.width), "--spp", str(a.spp), "--tolerance", str(a.tolerance)],
                       env=env, capture_output=True, text=True, timeout=420)
    if r.returncode != 0:
        raise RuntimeError(f"the child failed ({r.returncode}):\n{r.stderr[-2000:]}")
    info = json.loads(r.stdout.strip().splitlines()[-1])
    calls = {True: [], False: []}
    cur = None
    for ln in r.stderr.splitlines():
        m = LINE.match(ln.strip())
        if not m:
            continue
        guided, kind, step, final, ms = bool(m.group(1)), m.group(2), m.group(3), m.group(4), float(m.group(5))
        if kind == "prepare":
            cur = {"prepare": ms, "levels": []}
        elif kind == "level":
            cur["levels"].append((int(step), int(final), ms))
        else:
            cur["total"] = ms
            calls[guided].append(cur)
    n_pix = info["width"] * info["height"]
    hbm = lambda b: round(n_pix * b / (HBM_TBS * 1e12) * 1e3, 5)
    res = {"tool": "tools/gpu_accum_denoise.py", "warmup": WARMUP, "reps": REPS, "levels": LEVELS, "hbm_tb_s": HBM_TBS,
           "time": "feature pass: rtw_stats kernel_ms; noise map: stream events around the call; filter kernels: HIP events around each kernel "
                   "(RTW_DENOISE_PROFILE); median of the calls after warm-up, guided and plain alternating in one process"}
    res["frame"] = {k: info[k] for k in info if k not in ("feature_ms", "noise_ms")}
    res["tile_prefix_features"] = dict(med(info["feature_ms"]), compulsory_hbm_ms=hbm(32))
    res["noise_map"] = dict(med(info["noise_ms"]), compulsory_hbm_ms=hbm(68))
    for guided, name in ((True, "guided"), (False, "plain")):
        cs = calls[guided][WARMUP:]
        assert len(cs) == REPS, (name, len(cs))
        out = {"prepare": dict(med([c["prepare"] for c in cs]), compulsory_hbm_ms=hbm(44 + 48 + (4 if guided else 0))), "total": med([c["total"] for c in cs]),
               "per_level": []}
        for k in range(LEVELS):
            step, final, _ = cs[0]["levels"][k]
            ms = [c["levels"][k][2] for c in cs]
            b = 32 + (16 if guided else 0) + (12 if final else 16) + (16 if final and not guided else 0)
            out["per_level"].append(dict(med(ms), step=step, final=bool(final), compulsory_hbm_ms=hbm(b), times_hbm_bound=round(statistics.median(ms) / hbm(b), 2)))
        res[name] = out
    for k in ("tile_prefix_features", "noise_map"):
        res[k]["times_hbm_bound"] = round(res[k]["ms_median"] / res[k]["compulsory_hbm_ms"], 2)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
