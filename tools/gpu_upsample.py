#!/usr/bin/env python3
"""The feature-guided upsampler on one MI355X (include/rtw_hip.h rtw_upsample_*): the measurements of DESIGN.md 7.16.
usage: python tools/gpu_upsample.py [--reps 25] [--warmup 5] [--width 1920] [--out profiles/upsample_frames.json]

Each configuration runs in a fresh child process of this script, one at a time; every figure is the median of --reps repetitions after
--warmup.  Scene: scene_random_spheres through t_cam1, Float32, 4 spp.
  kernel   the device form at (width/2) -> width (960x540 -> 1920x1080), kernel by kernel: HIP events recorded by the library itself under
           the measurement aids RTW_ENABLE_TEST_AIDS=1 RTW_DENOISE_PROFILE=1 (one `[rtw upsample]` line per kernel on stderr; the call then
           blocks).  Next to it one dn_level launch at the full size (the denoiser's first level there, from its `[rtw denoise]` lines), and
           the upsampling kernel as a multiple of what its compulsory HBM bytes would take at 6.3 TB/s: features in 32 B and image out 12 B
           per full pixel, the E, G and A slots 48 B per small pixel, once.
  call     rtw_render_upsampled_f32 (width/2 -> width) against rtw_render_denoised_f32 at width: wall clock around the blocking call, and the
           RMSE of the linear result against a 1024-spp render at width.
  batch    64 previews of 48x27 -> 96x54 through rtw_render_upsampled_batch_f32 against 64 single calls: wall clock."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3
UP_LINE = re.compile(r"^\[rtw upsample\] f32 \S+ (prepare|level|upsample|total)(?: step=(\d+))?(?: levels=\d+)? ms=([0-9.]+)$")
DN_LINE = re.compile(r"^\[rtw denoise\] f32 \d+x\d+ level step=1 final=0 ms=([0-9.]+)$")


def _scene(R, T):
    R.reseed()
    return R.scene_random_spheres(elem_type=T), R.t_cam1(elem_type=T)


def child_kernel(a):
    import numpy as np
    import torch                             # (torch's HIP runtime first: INTEGRATION.md section 5)
    import rtw_amd as R
    from rtw_amd import _capi
    torch.cuda.init()
    L, T = _capi.lib(), np.float32
    W, H = a.width, R.image_height(a.width)
    w = (W + 1) // 2
    h = R.image_height(w)
    scene, cam_o = _scene(R, T)
    S, keep = _capi.make_scene(R.flatten_scene(scene, T), T)
    cam = _capi.make_camera(cam_o, T)
    handle = C.c_void_p()
    _capi.check(L.rtw_scene_upload_f32(C.byref(S), 0, C.byref(handle)))
    buf = lambda n: torch.empty(n, dtype=torch.float32, device="cuda:0")
    d_lo, d_flo, d_fhi, d_hi, d_out = buf(w * h * 3), buf(w * h * 8), buf(W * H * 8), buf(W * H * 3), buf(W * H * 3)
    d_work = buf(R.denoise_work_bytes(W, H, T) // 4)          # (the full-size denoiser's: larger than the upsampler's)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(stream.cuda_stream)
    P_lo, P_hi = _capi.make_params(w, h, 4, 16, 1, 4, gamma=0), _capi.make_params(W, H, 4, 16, 1, 4, gamma=0)
    _capi.check(L.rtw_render_device_f32(handle, C.byref(cam), C.byref(P_lo), ptr(d_lo), st))
    _capi.check(L.rtw_render_features_device_f32(handle, C.byref(cam), C.byref(P_lo), 0, 4, ptr(d_flo), st))
    _capi.check(L.rtw_render_features_device_f32(handle, C.byref(cam), C.byref(P_hi), 0, 4, ptr(d_fhi), st))
    _capi.check(L.rtw_render_device_f32(handle, C.byref(cam), C.byref(P_hi), ptr(d_hi), st))
    stream.synchronize()
    for _ in range(a.warmup + a.reps):
        R.upsample_into(d_out.data_ptr(), d_lo.data_ptr(), d_flo.data_ptr(), d_fhi.data_ptr(), d_work.data_ptr(), w, h, W, H, elem_type=T,
                        stream=stream.cuda_stream, gamma=False)
    stream.synchronize()
    nan_values = int(torch.isnan(d_out).sum().item())
    for _ in range(a.warmup + a.reps):
        R.denoise_into(d_out.data_ptr(), d_hi.data_ptr(), d_fhi.data_ptr(), d_work.data_ptr(), W, H, elem_type=T, stream=stream.cuda_stream, levels=3)
    stream.synchronize()
    L.rtw_scene_free(handle)
    del keep
    print(json.dumps({"lo": [w, h], "hi": [W, H], "nan_values": nan_values}))
    return 0


def _timed(fn, a):
    ms = []
    for _ in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = ms[a.warmup:]
    return out, {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}


def child_call(a):
    import numpy as np
    import torch
    import rtw_amd as R
    torch.cuda.init()
    T = np.float32
    scene, cam = _scene(R, T)
    W = a.width
    w = (W + 1) // 2
    truth = R.render(scene, cam, W, 1024, seed=99, gamma=False).astype(np.float64)
    up, t_up = _timed(lambda: R.render_upsampled(scene, cam, W, 4, lo_width=w, gamma=False), a)
    dn, t_dn = _timed(lambda: R.render_denoised(scene, cam, W, 4, gamma=False), a)
    raw, t_raw = _timed(lambda: R.render(scene, cam, W, 4, gamma=False), a)
    rmse = lambda x: round(float(np.sqrt(np.nanmean((x.astype(np.float64) - truth) ** 2))), 6)
    print(json.dumps({"lo_width": w, "width": W, "spp": 4, "truth_spp": 1024,
                      "render_upsampled": dict(t_up, rmse=rmse(up), nan_values=int(np.isnan(up).sum())),
                      "render_denoised": dict(t_dn, rmse=rmse(dn), nan_values=int(np.isnan(dn).sum())),
                      "render_plain": dict(t_raw, rmse=rmse(raw))}))
    return 0


def child_batch(a):
    import numpy as np
    import torch
    import rtw_amd as R
    torch.cuda.init()
    T = np.float32
    scene, cam = _scene(R, T)
    cams, seeds = [cam] * 64, list(range(1, 65))
    batch, t_b = _timed(lambda: R.render_upsampled_batch(scene, cams, 96, 4, seeds=seeds, lo_width=48, gamma=False), a)
    singles, t_s = _timed(lambda: [R.render_upsampled(scene, cam, 96, 4, seed=s, lo_width=48, gamma=False) for s in seeds], a)
    same = all(np.array_equal(batch[v].view(np.uint32), np.ascontiguousarray(singles[v]).view(np.uint32)) for v in range(64))
    print(json.dumps({"views": 64, "lo": [48, 27], "hi": [96, 54], "spp": 4, "batched_call": t_b, "single_calls": t_s, "views_equal_single_calls": bool(same)}))
    return 0


def run_config(a, name):
    env = dict(os.environ)
    if name == "kernel":
        env.update(RTW_ENABLE_TEST_AIDS="1", RTW_DENOISE_PROFILE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--warmup", str(a.warmup), "--width", str(a.width)],
                       env=env, capture_output=True, text=True, timeout=500)
    if r.returncode != 0:
        raise RuntimeError(f"{name}: the child failed ({r.returncode}):\n{r.stderr[-2000:]}")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    if name == "kernel":
        calls, cur, dn = [], None, []
        for ln in r.stderr.splitlines():
            m = UP_LINE.match(ln.strip())
            if m:
                kind, step, ms = m.group(1), m.group(2), float(m.group(3))
                if kind == "prepare":
                    cur = {"prepare": ms, "levels": []}
                elif kind == "level":
                    cur["levels"].append(ms)
                elif kind == "upsample":
                    cur["upsample"] = ms
                else:
                    cur["total"] = ms
                    calls.append(cur)
                continue
            m = DN_LINE.match(ln.strip())
            if m:
                dn.append(float(m.group(1)))
        calls, dn = calls[a.warmup:], dn[a.warmup:]
        assert len(calls) == a.reps and len(dn) == a.reps, (len(calls), len(dn))
        med = lambda xs: round(statistics.median(xs), 5)
        (w, h), (W, H) = res["lo"], res["hi"]
        hbm_ms = (W * H * (32 + 12) + w * h * 48) / (HBM_TBS * 1e12) * 1e3
        up = [c["upsample"] for c in calls]
        res.update(calls=len(calls), prepare_ms_median=med(c["prepare"] for c in calls), level_ms_median=[med(c["levels"][k] for c in calls) for k in range(2)],
                   upsample_ms_median=med(up), upsample_ms_min_max=[round(min(up), 5), round(max(up), 5)], total_ms_median=med(c["total"] for c in calls),
                   compulsory_hbm_ms=round(hbm_ms, 5), times_hbm_bound=round(statistics.median(up) / hbm_ms, 2),
                   dn_level_full_size_ms_median=med(dn), upsample_over_dn_level=round(statistics.median(up) / statistics.median(dn), 3))
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--child", default="")
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample_frames.json"))
    a = ap.parse_args()
    if a.child:
        return {"kernel": child_kernel, "call": child_call, "batch": child_batch}[a.child](a)
    res = {"tool": "tools/gpu_upsample.py", "reps": a.reps, "warmup": a.warmup, "hbm_tb_s": HBM_TBS,
           "time": "kernel: HIP events around each kernel (RTW_DENOISE_PROFILE); call, batch: wall clock around the blocking call; medians after warm-up",
           "configs": {}}
    for name in ("kernel", "call", "batch"):
        if not a.only or a.only == name:
            res["configs"][name] = run_config(a, name)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
