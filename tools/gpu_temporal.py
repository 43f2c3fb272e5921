#!/usr/bin/env python3
"""The temporal reprojection on one MI355X (include/rtw_hip.h rtw_temporal_*, rtw_render_sequence_*): the measurements of DESIGN.md 7.18.
usage: python tools/gpu_temporal.py [--reps 25] [--warmup 5] [--out profiles/temporal_frames.json]

Each configuration runs in a fresh child process of this script, one at a time; every figure is the median of --reps repetitions after
--warmup.  Scene: scene_random_spheres, two pinhole cameras a degree of orbit apart, 1 spp.
  kernel     the step kernel of the device form at 96x54, 480x270 and 1920x1080, Float32 and Float64: HIP events recorded by the library itself
             under the measurement aids RTW_ENABLE_TEST_AIDS=1 RTW_TEMPORAL_PROFILE=1 RTW_DENOISE_PROFILE=1 (one `[rtw temporal]` line per launch on stderr; the call
             then blocks).  Next to it, in the same process, one dn_level launch of the same frame (the denoiser's first level, from its
             `[rtw denoise]` lines), and the step as a multiple of what its compulsory HBM bytes would take at 6.3 TB/s: per pixel the image
             (3 elements) and the features (8) in, the previous state (9) in, the next state (9) and the image (3) out -- 32 elements.
  sequence   rtw_render_sequence_* with a filter for 16 views of 96x54 and of 480x270 at 1 spp against the same 16 views through
             rtw_render_filtered_batch_*: wall clock around the blocking call.  The difference is what the 16 sequential step launches cost."""
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
TP_LINE = re.compile(r"^\[rtw temporal\] (f32|f64) (\d+)x(\d+) step prev=([01]) paths=0 ms=([0-9.]+)$")
DN_LINE = re.compile(r"^\[rtw denoise\] (f32|f64) (\d+)x(\d+) level step=1 final=0 ms=([0-9.]+)$")
WIDTHS = (96, 480, 1920)


def _orbit(R, T, n, step_deg=1.0):
    import numpy as np
    cams = []
    for v in range(n):
        a = np.deg2rad(step_deg * v)
        cams.append(R.default_camera(lookfrom=(13 * np.cos(a) + 3 * np.sin(a), 2, -13 * np.sin(a) + 3 * np.cos(a)), lookat=(0, 0, 0), vfov=20, aperture=0,
                                     focus_dist=10, elem_type=T))
    return cams


def child_kernel(a):
    import numpy as np
    import torch                             # (torch's HIP runtime first: INTEGRATION.md section 5)
    import rtw_amd as R
    from rtw_amd import _capi
    torch.cuda.init()
    L = _capi.lib()
    accepted = {}
    for T, sfx, dt in ((np.float32, "f32", torch.float32), (np.float64, "f64", torch.float64)):
        R.reseed()
        scene = R.scene_random_spheres(elem_type=T)
        cams = _orbit(R, T, 2)
        S, keep = _capi.make_scene(R.flatten_scene(scene, T), T)
        handle = C.c_void_p()
        _capi.check(getattr(L, "rtw_scene_upload_" + sfx)(C.byref(S), 0, C.byref(handle)))
        for W in WIDTHS:
            H = R.image_height(W)
            buf = lambda n: torch.zeros(n, dtype=dt, device="cuda:0")
            img, feat = [buf(W * H * 3) for _ in range(2)], [buf(W * H * 8) for _ in range(2)]
            n_state = R.temporal_state_bytes(W, H, T) // np.dtype(T).itemsize
            s0, s1, out = buf(n_state), buf(n_state), buf(W * H * 3)
            work = buf(R.denoise_work_bytes(W, H, T) // np.dtype(T).itemsize)
            stream = torch.cuda.Stream()
            torch.cuda.synchronize()
            st = C.c_void_p(stream.cuda_stream)
            ptr = lambda t: C.c_void_p(t.data_ptr())
            P = _capi.make_params(W, H, 1, 16, 1, 1, gamma=0)
            for v in range(2):
                cm = _capi.make_camera(cams[v], T)
                P.seed = 1 + v
                _capi.check(getattr(L, "rtw_render_device_" + sfx)(handle, C.byref(cm), C.byref(P), ptr(img[v]), st))
                _capi.check(getattr(L, "rtw_render_features_device_" + sfx)(handle, C.byref(cm), C.byref(P), 0, 1, ptr(feat[v]), st))
            stream.synchronize()
            kw = dict(elem_type=T, stream=stream.cuda_stream, gamma=False)
            R.temporal_step_into(out.data_ptr(), s0.data_ptr(), img[0].data_ptr(), feat[0].data_ptr(), cams[0], W, H, **kw)         # the first frame: prev=0
            for _ in range(a.warmup + a.reps):
                R.temporal_step_into(out.data_ptr(), s1.data_ptr(), img[1].data_ptr(), feat[1].data_ptr(), cams[1], W, H, d_state_prev_ptr=s0.data_ptr(),
                                     cam_prev=cams[0], **kw)
            stream.synchronize()
            accepted[f"{sfx} {W}x{H}"] = round(float((s1[8 * W * H:9 * W * H] > 1).float().mean().item()), 4)
            for _ in range(a.warmup + a.reps):
                R.denoise_into(out.data_ptr(), img[1].data_ptr(), feat[1].data_ptr(), work.data_ptr(), W, H, elem_type=T, stream=stream.cuda_stream, levels=2)
            stream.synchronize()
        getattr(L, "rtw_scene_free")(handle)
        del keep
    print(json.dumps({"accepted_share": accepted}))
    return 0


def _timed(fn, a):
    ms = []
    for _ in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = ms[a.warmup:]
    return out, {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}


def child_sequence(a):
    import numpy as np
    import torch
    import rtw_amd as R
    torch.cuda.init()
    res = {}
    for T in (np.float32, np.float64):
        R.reseed()
        scene = R.scene_random_spheres(elem_type=T)
        cams, seeds = _orbit(R, T, 16), list(range(1, 17))
        for W in (96, 480):
            seq, t_seq = _timed(lambda: R.render_sequence(scene, cams, W, 1, seeds=seeds, denoise=True, gamma=False), a)
            flt, t_flt = _timed(lambda: R.render_denoised_batch(scene, cams, W, 1, seeds=seeds, gamma=False), a)
            plain, t_seq0 = _timed(lambda: R.render_sequence(scene, cams, W, 1, seeds=seeds, gamma=False), a)
            res[f"{np.dtype(T).name} {W}x{R.image_height(W)}"] = {
                "views": 16, "spp": 1, "render_sequence_filtered": t_seq, "render_filtered_batch": t_flt, "render_sequence_unfiltered": t_seq0,
                "sequence_minus_batch_ms": round(t_seq["ms_median"] - t_flt["ms_median"], 4),
                "per_step_ms": round((t_seq["ms_median"] - t_flt["ms_median"]) / 16, 5),
                "nan_values": int(np.isnan(seq).sum()) + int(np.isnan(plain).sum()),
                "view_0_differs_from_batch_only_by_rounding": bool(np.allclose(seq[0], flt[0], rtol=0, atol=1e-4))}
    print(json.dumps(res))
    return 0


def run_config(a, name):
    env = dict(os.environ)
    if name == "kernel":
        env.update(RTW_ENABLE_TEST_AIDS="1", RTW_TEMPORAL_PROFILE="1", RTW_DENOISE_PROFILE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                       env=env, capture_output=True, text=True, timeout=500)
    if r.returncode != 0:
        raise RuntimeError(f"{name}: the child failed ({r.returncode}):\n{r.stderr[-2000:]}")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    if name == "kernel":
        tp, dn = {}, {}
        for ln in r.stderr.splitlines():
            m = TP_LINE.match(ln.strip())
            if m and m.group(4) == "1":
                tp.setdefault((m.group(1), int(m.group(2)), int(m.group(3))), []).append(float(m.group(5)))
                continue
            m = DN_LINE.match(ln.strip())
            if m:
                dn.setdefault((m.group(1), int(m.group(2)), int(m.group(3))), []).append(float(m.group(4)))
        frames = {}
        for key in sorted(tp):
            sfx, W, H = key
            t, d = tp[key][a.warmup:], dn[key][a.warmup:]
            assert len(t) == a.reps and len(d) == a.reps, (key, len(t), len(d))
            hbm_ms = W * H * 32 * (8 if sfx == "f64" else 4) / (HBM_TBS * 1e12) * 1e3
            frames[f"{sfx} {W}x{H}"] = {"step_ms_median": round(statistics.median(t), 5), "step_ms_min_max": [round(min(t), 5), round(max(t), 5)],
                                        "dn_level_ms_median": round(statistics.median(d), 5), "step_over_dn_level": round(statistics.median(t) / statistics.median(d), 3),
                                        "compulsory_hbm_ms": round(hbm_ms, 6), "times_hbm_bound": round(statistics.median(t) / hbm_ms, 2)}
        res["frames"] = frames
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", default="")
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_frames.json"))
    a = ap.parse_args()
    if a.child:
        return {"kernel": child_kernel, "sequence": child_sequence}[a.child](a)
    res = {"tool": "tools/gpu_temporal.py", "reps": a.reps, "warmup": a.warmup, "hbm_tb_s": HBM_TBS,
           "time": "kernel: HIP events around each kernel (RTW_TEMPORAL_PROFILE, RTW_DENOISE_PROFILE); sequence: wall clock around the blocking call; medians after warm-up",
           "configs": {}}
    for name in ("kernel", "sequence"):
        if not a.only or a.only == name:
            res["configs"][name] = run_config(a, name)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
