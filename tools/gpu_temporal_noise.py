#!/usr/bin/env python3
"""The temporal moments on one MI355X (include/rtw_hip.h rtw_history_moments_*, rtw_history_noise_device_*, rtw_render_path_guided_*):
the measurements of DESIGN.md 7.19.
usage: python tools/gpu_temporal_noise.py [--reps 25] [--warmup 5] [--out profiles/temporal_noise_frames.json]

Each configuration runs in a fresh child process of this script, one at a time; every figure is the median of --reps repetitions after
--warmup.  Scene: scene_random_spheres, two pinhole cameras a degree of orbit apart, 1 spp (the frames of tools/gpu_temporal.py).
  kernel     at 96x54, 480x270 and 1920x1080, Float32 and Float64, HIP events recorded by the library itself under the measurement aids
             RTW_ENABLE_TEST_AIDS=1 RTW_TEMPORAL_PROFILE=1 (one `[rtw temporal]` line per launch on stderr; the call then blocks):
             the step with moments next to the plain step in the same process, and the noise kernel at radius 1, 2, 3 over a state whose
             history lengths are all 8 (>= min_len = 4: no lane walks the window) and over the same state with all lengths 1 (every lane
             does).  Each as a multiple of what its compulsory HBM bytes would take at 6.3 TB/s: per pixel the step moves 34 elements
             (the plain step's 32 and M in and out), the map 10 in (E, G, L, M) and 1 out.
  sequence   rtw_render_path_guided_* for 16 views of 96x54 and of 480x270 at 1 spp against rtw_render_sequence_* with the plain
             filter: wall clock around the blocking call.  The difference is 16 noise launches, the moments and the guided kernels."""
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
STEP_LINE = re.compile(r"^\[rtw temporal\] (f32|f64) (\d+)x(\d+) (step|step\+moments) prev=1 paths=0 ms=([0-9.]+)$")
NOISE_LINE = re.compile(r"^\[rtw temporal\] (f32|f64) (\d+)x(\d+) noise r=(\d) paths=0 ms=([0-9.]+)$")
WIDTHS = (96, 480, 1920)
RADII = (1, 2, 3)


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
    for T, sfx, dt in ((np.float32, "f32", torch.float32), (np.float64, "f64", torch.float64)):
        R.reseed()
        scene = R.scene_random_spheres(elem_type=T)
        cams = _orbit(R, T, 2)
        S, keep = _capi.make_scene(R.flatten_scene(scene, T), T)
        handle = C.c_void_p()
        _capi.check(getattr(L, "rtw_scene_upload_" + sfx)(C.byref(S), 0, C.byref(handle)))
        for W in WIDTHS:
            H = R.image_height(W)
            eb = np.dtype(T).itemsize
            buf = lambda n: torch.zeros(n, dtype=dt, device="cuda:0")
            img, feat = [buf(W * H * 3) for _ in range(2)], [buf(W * H * 8) for _ in range(2)]
            n_state, n_mom = R.temporal_state_bytes(W, H, T) // eb, R.temporal_moment_bytes(W, H, T) // eb
            s0, s1, m0, m1, out, rho = buf(n_state), buf(n_state), buf(n_mom), buf(n_mom), buf(W * H * 3), buf(W * H)
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
            R.temporal_step_moments_into(out.data_ptr(), s0.data_ptr(), m0.data_ptr(), img[0].data_ptr(), feat[0].data_ptr(), cams[0], W, H, **kw)      # the first frame
            for _ in range(a.warmup + a.reps):                  # the plain step and the step with moments, alternating
                R.temporal_step_into(out.data_ptr(), s1.data_ptr(), img[1].data_ptr(), feat[1].data_ptr(), cams[1], W, H, d_state_prev_ptr=s0.data_ptr(), cam_prev=cams[0], **kw)
                R.temporal_step_moments_into(out.data_ptr(), s1.data_ptr(), m1.data_ptr(), img[1].data_ptr(), feat[1].data_ptr(), cams[1], W, H, d_state_prev_ptr=s0.data_ptr(),
                                             d_moment_prev_ptr=m0.data_ptr(), cam_prev=cams[0], **kw)
            stream.synchronize()
            for length in (8.0, 1.0):                           # all histories long, then all short (slots that are not valid keep len 0)
                lens = s1[8 * W * H:9 * W * H]
                lens.copy_(torch.where(lens > 0, torch.full_like(lens, length), lens))
                torch.cuda.synchronize()
                for r in RADII:
                    for _ in range(a.warmup + a.reps):
                        R.temporal_noise_into(rho.data_ptr(), s1.data_ptr(), m1.data_ptr(), W, H, elem_type=T, stream=stream.cuda_stream, radius=r)
                stream.synchronize()
        getattr(L, "rtw_scene_free")(handle)
        del keep
    print(json.dumps({}))
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
            gd, t_gd = _timed(lambda: R.render_sequence(scene, cams, W, 1, seeds=seeds, guided=True, gamma=False), a)
            pl, t_pl = _timed(lambda: R.render_sequence(scene, cams, W, 1, seeds=seeds, denoise=True, gamma=False), a)
            res[f"{np.dtype(T).name} {W}x{R.image_height(W)}"] = {
                "views": 16, "spp": 1, "render_sequence_guided": t_gd, "render_sequence_filtered": t_pl,
                "guided_minus_plain_ms": round(t_gd["ms_median"] - t_pl["ms_median"], 4), "per_view_ms": round((t_gd["ms_median"] - t_pl["ms_median"]) / 16, 5),
                "nan_values": int(np.isnan(gd).sum()) + int(np.isnan(pl).sum())}
    print(json.dumps(res))
    return 0


def run_config(a, name):
    env = dict(os.environ)
    if name == "kernel":
        env.update(RTW_ENABLE_TEST_AIDS="1", RTW_TEMPORAL_PROFILE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                       env=env, capture_output=True, text=True, timeout=500)
    if r.returncode != 0:
        raise RuntimeError(f"{name}: the child failed ({r.returncode}):\n{r.stderr[-2000:]}")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    if name == "kernel":
        steps, noise = {}, {}
        for ln in r.stderr.splitlines():
            m = STEP_LINE.match(ln.strip())
            if m:
                steps.setdefault((m.group(1), int(m.group(2)), int(m.group(3)), m.group(4)), []).append(float(m.group(5)))
                continue
            m = NOISE_LINE.match(ln.strip())
            if m:
                noise.setdefault((m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))), []).append(float(m.group(5)))
        n_run = a.warmup + a.reps
        med = lambda v: round(statistics.median(v), 5)
        frames = {}
        for sfx, W, H in sorted({k[:3] for k in steps}):
            eb = 8 if sfx == "f64" else 4
            plain, mom = steps[(sfx, W, H, "step")][a.warmup:], steps[(sfx, W, H, "step+moments")][a.warmup:]
            assert len(plain) == a.reps and len(mom) == a.reps, (sfx, W, H, len(plain), len(mom))
            hbm_step, hbm_map = (W * H * k * eb / (HBM_TBS * 1e12) * 1e3 for k in (34, 11))
            row = {"plain_step_ms_median": med(plain), "plain_step_ms_min_max": [round(min(plain), 5), round(max(plain), 5)],
                   "moment_step_ms_median": med(mom), "moment_step_ms_min_max": [round(min(mom), 5), round(max(mom), 5)],
                   "moment_over_plain": round(statistics.median(mom) / statistics.median(plain), 3),
                   "step_compulsory_hbm_ms": round(hbm_step, 6), "moment_step_times_hbm_bound": round(statistics.median(mom) / hbm_step, 2),
                   "map_compulsory_hbm_ms": round(hbm_map, 6), "noise": {}}
            for r_ in RADII:
                t = noise[(sfx, W, H, r_)]
                assert len(t) == 2 * n_run, (sfx, W, H, r_, len(t))
                long_, short = t[a.warmup:n_run], t[n_run + a.warmup:]
                row["noise"][f"radius {r_}"] = {"all_long_ms_median": med(long_), "all_long_times_hbm_bound": round(statistics.median(long_) / hbm_map, 2),
                                                "all_short_ms_median": med(short), "all_short_times_hbm_bound": round(statistics.median(short) / hbm_map, 2)}
            frames[f"{sfx} {W}x{H}"] = row
        res["frames"] = frames
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", default="")
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_noise_frames.json"))
    a = ap.parse_args()
    if a.child:
        return {"kernel": child_kernel, "sequence": child_sequence}[a.child](a)
    res = {"tool": "tools/gpu_temporal_noise.py", "reps": a.reps, "warmup": a.warmup, "hbm_tb_s": HBM_TBS,
           "time": "kernel: HIP events around each kernel (RTW_TEMPORAL_PROFILE); sequence: wall clock around the blocking call; medians after warm-up",
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
