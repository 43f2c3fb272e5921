#!/usr/bin/env python3
"""The present stage on one MI355X (include/rtw_hip.h rtw_present_*, rtw_render_presented_*): the measurements of DESIGN.md 7.20.
usage: python tools/gpu_present.py [--reps 25] [--warmup 5] [--out profiles/present_frames.json]

Each configuration runs in a fresh child process of this script, one at a time; every figure is the median of --reps repetitions after
--warmup.  Scene: scene_random_spheres, 1 spp.
  kernel      the present kernel of the device form at 96x54, 480x270 and 1920x1080 (and 1919x1080: the unaligned-row path of C = 3), Float32 and
              Float64, C = 3 and C = 4: HIP events recorded by the library itself under the measurement aids RTW_ENABLE_TEST_AIDS=1
              RTW_PRESENT_PROFILE=1 RTW_DENOISE_PROFILE=1 (one `[rtw present]` line per launch on stderr; the call then blocks).  Next to it, in the
              same process, one dn_level launch of the same frame (the denoiser's first level, from its `[rtw denoise]` lines), and the kernel as
              a multiple of what its compulsory HBM bytes would take at 6.3 TB/s: per pixel 3 elements in and C bytes out.
  end_to_end  wall clock around the blocking calls, 16 views of 480x270 and one view of 1920x1080: render_presented_batch / render_presented
              against render_batch / render followed by imageio.to_u8 on the result, in the same process; the D2H bytes of both; the host
              conversion alone (whatever this host's CPU makes of it)."""
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
PR_LINE = re.compile(r"^\[rtw present\] (f32|f64) (\d+)x(\d+) views=1 C=([34]) (dword|aligned|unaligned) ms=([0-9.]+)$")
DN_LINE = re.compile(r"^\[rtw denoise\] (f32|f64) (\d+)x(\d+) level step=1 final=0 ms=([0-9.]+)$")
FRAMES = ((96, 54), (480, 270), (1920, 1080))


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
        cam = R.t_cam1(elem_type=T)
        S, keep = _capi.make_scene(R.flatten_scene(scene, T), T)
        handle = C.c_void_p()
        _capi.check(getattr(L, "rtw_scene_upload_" + sfx)(C.byref(S), 0, C.byref(handle)))
        for W, H in FRAMES:
            buf = lambda n: torch.zeros(n, dtype=dt, device="cuda:0")
            img, feat, out = buf(W * H * 3), buf(W * H * 8), buf(W * H * 3)
            work = buf(R.denoise_work_bytes(W, H, T) // np.dtype(T).itemsize)
            u8 = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda:0")
            stream = torch.cuda.Stream()
            torch.cuda.synchronize()
            st = C.c_void_p(stream.cuda_stream)
            ptr = lambda t: C.c_void_p(t.data_ptr())
            P = _capi.make_params(W, H, 1, 16, 1, 1, gamma=1)
            cm = _capi.make_camera(cam, T)
            _capi.check(getattr(L, "rtw_render_device_" + sfx)(handle, C.byref(cm), C.byref(P), ptr(img), st))
            _capi.check(getattr(L, "rtw_render_features_device_" + sfx)(handle, C.byref(cm), C.byref(P), 0, 1, ptr(feat), st))
            stream.synchronize()
            for w in ((W, W - 1) if W == 1920 else (W,)):                  # (W - 1: the same buffer read as a frame one column narrower)
                for channels in (3, 4):
                    for _ in range(a.warmup + a.reps):
                        R.present_into(u8.data_ptr(), img.data_ptr(), w, H, elem_type=T, stream=stream.cuda_stream, channels=channels)
            stream.synchronize()
            for _ in range(a.warmup + a.reps):
                R.denoise_into(out.data_ptr(), img.data_ptr(), feat.data_ptr(), work.data_ptr(), W, H, elem_type=T, stream=stream.cuda_stream, levels=2)
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


def child_end_to_end(a):
    import numpy as np
    import torch
    import rtw_amd as R
    torch.cuda.init()
    res = {}
    for T in (np.float32, np.float64):
        R.reseed()
        scene = R.scene_random_spheres(elem_type=T)
        cams, seeds = [R.t_cam1(elem_type=T)] * 16, list(range(1, 17))
        eb = np.dtype(T).itemsize
        u8, t_new = _timed(lambda: R.render_presented_batch(scene, cams, 480, 1, seeds=seeds), a)
        flt, t_render = _timed(lambda: R.render_batch(scene, cams, 480, 1, seed=seeds), a)
        ref, t_conv = _timed(lambda: R.imageio.to_u8(flt), a)
        res[f"{np.dtype(T).name} 16 x 480x270"] = {
            "render_presented_batch": t_new, "render_batch": t_render, "to_u8_on_this_host": t_conv,
            "render_batch_then_to_u8_ms": round(t_render["ms_median"] + t_conv["ms_median"], 4),
            "d2h_bytes_presented": 16 * 480 * 270 * 3, "d2h_bytes_float": 16 * 480 * 270 * 3 * eb, "same_bytes": bool(np.array_equal(u8, ref))}
        u8, t_new = _timed(lambda: R.render_presented(scene, cams[0], 1920, 1), a)
        flt, t_render = _timed(lambda: R.render(scene, cams[0], 1920, 1), a)
        ref, t_conv = _timed(lambda: R.imageio.to_u8(flt), a)
        res[f"{np.dtype(T).name} 1 x 1920x1080"] = {
            "render_presented": t_new, "render": t_render, "to_u8_on_this_host": t_conv,
            "render_then_to_u8_ms": round(t_render["ms_median"] + t_conv["ms_median"], 4),
            "d2h_bytes_presented": 1920 * 1080 * 3, "d2h_bytes_float": 1920 * 1080 * 3 * eb, "same_bytes": bool(np.array_equal(u8, ref))}
    print(json.dumps(res))
    return 0


def run_config(a, name):
    env = dict(os.environ)
    if name == "kernel":
        env.update(RTW_ENABLE_TEST_AIDS="1", RTW_PRESENT_PROFILE="1", RTW_DENOISE_PROFILE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                       env=env, capture_output=True, text=True, timeout=500)
    if r.returncode != 0:
        raise RuntimeError(f"{name}: the child failed ({r.returncode}):\n{r.stderr[-2000:]}")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    if name == "kernel":
        pr, dn = {}, {}
        for ln in r.stderr.splitlines():
            m = PR_LINE.match(ln.strip())
            if m:
                pr.setdefault((m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), m.group(5)), []).append(float(m.group(6)))
                continue
            m = DN_LINE.match(ln.strip())
            if m:
                dn.setdefault((m.group(1), int(m.group(2)), int(m.group(3))), []).append(float(m.group(4)))
        frames = {}
        for key in sorted(pr):
            sfx, W, H, ch, path = key
            t, d = pr[key][a.warmup:], dn[(sfx, W if W != 1919 else 1920, H)][a.warmup:]
            assert len(t) == a.reps and len(d) == a.reps, (key, len(t), len(d))
            hbm_ms = W * H * (3 * (8 if sfx == "f64" else 4) + ch) / (HBM_TBS * 1e12) * 1e3
            frames[f"{sfx} {W}x{H} C={ch} {path}"] = {
                "present_ms_median": round(statistics.median(t), 5), "present_ms_min_max": [round(min(t), 5), round(max(t), 5)],
                "dn_level_ms_median": round(statistics.median(d), 5), "present_over_dn_level": round(statistics.median(t) / statistics.median(d), 3),
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "present_frames.json"))
    a = ap.parse_args()
    if a.child:
        return {"kernel": child_kernel, "end_to_end": child_end_to_end}[a.child](a)
    res = {"tool": "tools/gpu_present.py", "reps": a.reps, "warmup": a.warmup, "hbm_tb_s": HBM_TBS,
           "time": "kernel: HIP events around each kernel (RTW_PRESENT_PROFILE, RTW_DENOISE_PROFILE); end_to_end: wall clock around the blocking call; medians after warm-up",
           "configs": {}}
    for name in ("kernel", "end_to_end"):
        if not a.only or a.only == name:
            res["configs"][name] = run_config(a, name)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
