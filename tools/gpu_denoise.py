#!/usr/bin/env python3
"""The feature-guided denoiser on one MI355X (include/rtw_hip.h rtw_denoise_device_f32), kernel by kernel: the measurements of DESIGN.md 7.10.
usage: python tools/gpu_denoise.py [--reps 25] [--warmup 5] [--width 1920] [--out profiles/denoise_frames.json]

The frame: scene_random_spheres through t_cam1 at --width (1920 x 1080), Float32, 4 spp, linear (rtw_render_device_f32) and its feature
pass over all 4 chunks (rtw_render_features_device_f32) -- both timed by rtw_stats().kernel_ms, for orientation: the denoiser exists to be
cheaper than more samples.  The denoiser runs on those buffers with the defaults.

Time: HIP events around every kernel, recorded by the library itself under the measurement aids RTW_ENABLE_TEST_AIDS=1 RTW_DENOISE_PROFILE=1
(one line per kernel on stderr; the call then blocks).  Each configuration runs in a child process of this script (the aids are read once
per process), one at a time; per kernel the median of --reps calls after --warmup.  Configurations:
  levels_3, levels_5   levels = 3 and 5: steps 1, 2, 4 and 1, 2, 4, 8, 16, and the totals
Each level is also given as a multiple of what its compulsory HBM bytes would take at 6.3 TB/s: records in (32 B per pixel), colour out
(16 B; the last level: the albedo in, 16 B, and the image out, 12 B), once."""
import argparse
import ctypes as C
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3
LINE = re.compile(r"^\[rtw denoise\] f32 \d+x\d+ (prepare|level|total)(?: step=(\d+) final=(\d))?(?: levels=\d+)? ms=([0-9.]+)$")


def child(a):
    import numpy as np
    import torch                             # (torch's HIP runtime first: INTEGRATION.md section 5)
    import rtw_amd as R
    from rtw_amd import _capi
    torch.cuda.init()
    L = _capi.lib()
    T = np.float32
    width, height = a.width, R.image_height(a.width)
    R.reseed()
    flat = R.flatten_scene(R.scene_random_spheres(elem_type=T), T)
    S, keep = _capi.make_scene(flat, T)
    cam = _capi.make_camera(R.t_cam1(elem_type=T), T)
    handle = C.c_void_p()
    _capi.check(L.rtw_scene_upload_f32(C.byref(S), 0, C.byref(handle)))
    d_img = torch.empty(width * height * 3, dtype=torch.float32, device="cuda:0")
    d_feat = torch.empty(width * height * 8, dtype=torch.float32, device="cuda:0")
    d_out = torch.empty(width * height * 3, dtype=torch.float32, device="cuda:0")
    d_work = torch.empty(R.denoise_work_bytes(width, height, T) // 4, dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    P = _capi.make_params(width, height, 4, 16, 1, 4, gamma=0)

    def stats():
        st = _capi.Stats()
        _capi.check(L.rtw_stats(C.byref(st)))
        return st.kernel_ms

    render_ms, feature_ms = [], []
    for _ in range(3 + 7):
        _capi.check(L.rtw_render_device_f32(handle, C.byref(cam), C.byref(P), C.c_void_p(d_img.data_ptr()), C.c_void_p(stream.cuda_stream)))
        render_ms.append(stats())
        _capi.check(L.rtw_render_features_device_f32(handle, C.byref(cam), C.byref(P), 0, 4, C.c_void_p(d_feat.data_ptr()), C.c_void_p(stream.cuda_stream)))
        feature_ms.append(stats())
    for _ in range(a.warmup + a.reps):
        R.denoise_into(d_out.data_ptr(), d_img.data_ptr(), d_feat.data_ptr(), d_work.data_ptr(), width, height, elem_type=T, stream=stream.cuda_stream,
                       levels=a.levels)
    stream.synchronize()
    out = d_out.cpu().numpy()
    L.rtw_scene_free(handle)
    del keep
    print(json.dumps({"width": width, "height": height, "render_4spp_ms_median": round(statistics.median(render_ms[3:]), 4),
                      "features_4chunks_ms_median": round(statistics.median(feature_ms[3:]), 4), "sha256": hashlib.sha256(out.tobytes()).hexdigest(),
                      "nan_values": int(np.isnan(out).sum())}))
    return 0


def run_config(a, name, levels):
    env = dict(os.environ, RTW_ENABLE_TEST_AIDS="1", RTW_DENOISE_PROFILE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--levels", str(levels), "--reps", str(a.reps), "--warmup", str(a.warmup),
                        "--width", str(a.width)], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"{name}: the child failed ({r.returncode}):\n{r.stderr[-2000:]}")
    info = json.loads(r.stdout.strip().splitlines()[-1])
    calls, cur = [], None
    for ln in r.stderr.splitlines():
        m = LINE.match(ln.strip())
        if not m:
            continue
        kind, step, final, ms = m.group(1), m.group(2), m.group(3), float(m.group(4))
        if kind == "prepare":
            cur = {"prepare": ms, "levels": []}
        elif kind == "level":
            cur["levels"].append((int(step), int(final), ms))
        else:
            cur["total"] = ms
            calls.append(cur)
    calls = calls[a.warmup:]
    assert len(calls) == a.reps, (name, len(calls))
    n_pix = info["width"] * info["height"]
    res = {"levels": levels, "calls": len(calls), "prepare_ms_median": round(statistics.median(c["prepare"] for c in calls), 5),
           "total_ms_median": round(statistics.median(c["total"] for c in calls), 5),
           "total_ms_min_max": [round(min(c["total"] for c in calls), 5), round(max(c["total"] for c in calls), 5)], "per_level": []}
    for k in range(levels):
        step, final, _ = calls[0]["levels"][k]
        ms = [c["levels"][k][2] for c in calls]
        hbm_ms = n_pix * (32 + (28 if final else 16)) / (HBM_TBS * 1e12) * 1e3
        res["per_level"].append({"step": step, "final": bool(final), "ms_median": round(statistics.median(ms), 5),
                                 "ms_min_max": [round(min(ms), 5), round(max(ms), 5)], "compulsory_hbm_ms": round(hbm_ms, 5),
                                 "times_hbm_bound": round(statistics.median(ms) / hbm_ms, 2)})
    res.update(info)
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_frames.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"tool": "tools/gpu_denoise.py", "reps": a.reps, "warmup": a.warmup, "hbm_tb_s": HBM_TBS,
           "time": "HIP events around each kernel (RTW_DENOISE_PROFILE), median over the calls after warm-up", "configs": {}}
    for name, levels in (("levels_3", 3), ("levels_5", 5)):
        res["configs"][name] = run_config(a, name, levels)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0 if all(c["nan_values"] == 0 for c in res["configs"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
