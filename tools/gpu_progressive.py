#!/usr/bin/env python3
"""What progressive rendering costs (include/rtw_hip.h rtw_render_accum_*), on one MI355X.
usage: python tools/gpu_progressive.py [--reps 3] [--out profiles/progressive_frames.json] [--baseline-lib OTHER/librtw_hip.so]

  passes       the headline frame (scene_random_spheres, t_cam1, 1920 x 1080, 1000 spp = 250 chunks of 4, depth 50, Float32) rendered as
               1, 2, 5, 10, 25, 50 and 250 passes into one accumulator on one stream, the last pass writing the image -- against ONE
               rtw_render_device_f32 of the same frame (this library's, and with --baseline-lib another build's, e.g. the parent
               commit's, timed by a child process in the same session).  Per row: wall time (host clock from the first call to the end
               of a wait for the stream; median of --reps) and, from a second set of runs that asks rtw_stats() after every pass, the
               summed HIP-event kernel time.  The single render and the rows alternate within a repetition.
               Rows of 10 passes and more are also timed with the caller's job_pixels = 1, 4 and 16 (0 = the launcher's own rule).
  interactive  1 chunk of 1 sample per pass with the running image written, n_chunks = n_samples (open-ended refinement), at 320 x 180
               (BASELINE configs[1]'s size, depth 16) and at 1920 x 1080 (depth 50): passes per second, pipelined (the passes enqueued
               back to back, one wait at the end) and synchronous (a wait after every pass: a viewer that shows every image).
Every frame is checked against the one-shot render (sha256 of the frame bytes) BEFORE its time is recorded; a mismatch fails the run.
Kernel-level detail: run the tool under `rocprofv3 --kernel-trace --stats -- python tools/gpu_progressive.py ...`."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rtw_amd as R                      # noqa: E402
from rtw_amd import _capi                # noqa: E402

HEADLINE = dict(width=1920, spp=1000, depth=50)


class Frame:
    """scene_random_spheres through t_cam1 at one size, device-resident, on a stream of its own"""

    def __init__(self, L, width, spp, depth, n_chunks=0):
        import torch
        self.torch, self.L = torch, L
        T = np.float32
        self.width, self.height, self.spp, self.depth = width, R.image_height(width), spp, depth
        R.reseed()                                                # (the scene generator draws from the package's generator: the same 485 spheres every time)
        S, keep = _capi.make_scene(R.flatten_scene(R.scene_random_spheres(elem_type=T), T), T)
        self.cam = _capi.make_camera(R.t_cam1(elem_type=T), T)
        self.scene = C.c_void_p()
        self.check(L.rtw_scene_upload_f32(C.byref(S), 0, C.byref(self.scene)))
        self.P = _capi.make_params(width, self.height, spp, depth, 1, n_chunks)
        self.Pj = {jp: _capi.make_params(width, self.height, spp, depth, 1, n_chunks, job_pixels=jp) for jp in (0, 1, 4, 16)}
        self.buf = torch.zeros(width * self.height * 3, dtype=torch.float32, device="cuda:0")
        self.stream = torch.cuda.Stream()
        self.sp = C.c_void_p(self.stream.cuda_stream)

    def check(self, rc):
        if rc:
            raise RuntimeError(f"librtw_hip error {rc}: {self.L.rtw_last_error().decode()}")

    def stats(self):
        st = _capi.Stats()
        self.check(self.L.rtw_stats(C.byref(st)))
        return st

    def single(self):
        """-> (wall ms, kernel ms)"""
        t0 = time.perf_counter()
        self.check(self.L.rtw_render_device_f32(self.scene, C.byref(self.cam), C.byref(self.P), C.c_void_p(self.buf.data_ptr()), self.sp))
        st = self.stats()
        return (time.perf_counter() - t0) * 1e3, st.kernel_ms

    def hash(self):
        self.stream.synchronize()
        return hashlib.sha256(self.buf.cpu().numpy().tobytes()).hexdigest()

    def clear(self):
        self.buf.fill_(-1.0)
        self.torch.cuda.synchronize()


def bind_minimal(path):
    """another build of the library (one that may lack the rtw_accum_* symbols): only what the single render needs"""
    L = C.CDLL(path)
    L.rtw_last_error.restype = C.c_char_p
    L.rtw_scene_upload_f32.argtypes = [C.POINTER(_capi.SceneF32), C.c_int, C.POINTER(C.c_void_p)]
    L.rtw_render_device_f32.argtypes = [C.c_void_p, C.POINTER(_capi.CameraF32), C.POINTER(_capi.Params), C.c_void_p, C.c_void_p]
    L.rtw_stats.argtypes = [C.POINTER(_capi.Stats)]
    return L


def single_only(a):
    """child process of --baseline-lib: the one-shot render of the headline frame with another library, one JSON line"""
    import torch
    torch.cuda.init()
    f = Frame(bind_minimal(a.lib), **HEADLINE)
    f.single()
    ts = [f.single() for _ in range(a.reps)]
    print(json.dumps({"lib": a.lib, "wall_ms": [round(t[0], 3) for t in ts], "kernel_ms": [round(t[1], 3) for t in ts], "sha256": f.hash()}))
    return 0


def ranges(n_chunks, passes):
    return [(k * n_chunks // passes, (k + 1) * n_chunks // passes) for k in range(passes)]


def progressive(f, acc, n_chunks, passes, per_pass_stats, job_pixels=0):
    """one render in `passes` passes (the last writes the image) -> (wall ms, summed kernel ms or None)"""
    L = f.L
    f.check(L.rtw_accum_reset(acc, f.sp))
    f.stream.synchronize()
    kernel = 0.0
    t0 = time.perf_counter()
    for k, (b, e) in enumerate(ranges(n_chunks, passes)):
        out = C.c_void_p(f.buf.data_ptr()) if k == passes - 1 else None
        f.check(L.rtw_render_accum_f32(f.scene, C.byref(f.cam), C.byref(f.Pj[job_pixels]), b, e - b, acc, out, f.sp))
        if per_pass_stats:
            kernel += f.stats().kernel_ms
    f.stats()
    return (time.perf_counter() - t0) * 1e3, (kernel if per_pass_stats else None)


def med(xs):
    return round(statistics.median(xs), 3)


def spread(xs):
    return [round(min(xs), 3), round(max(xs), 3)]


def measure_passes(L, a, res):
    f = Frame(L, **HEADLINE)
    acc = C.c_void_p()
    f.check(L.rtw_accum_create(0, f.width, f.height, C.byref(acc)))
    n_chunks = 250
    f.single()
    ref = f.hash()
    rows = [1, 2, 5, 10, 25, 50, 250]
    ok = True
    for p in rows:                                   # the check first: every partition gives the one-shot frame
        f.clear()
        progressive(f, acc, n_chunks, p, False)
        same = f.hash() == ref
        ok &= same
        print(f"passes={p}: frame {'identical' if same else 'DIFFERS'}", flush=True)
    if not ok:
        return False
    single_t, wall, kern = [], {p: [] for p in rows}, {p: [] for p in rows}
    jp_rows = [p for p in rows if p >= 10]               # few chunks per pass: what the caller's job_pixels does to the row
    wall_jp = {(p, jp): [] for p in jp_rows for jp in (1, 4, 16)}
    for _ in range(a.reps):
        single_t.append(f.single())
        for p in rows:
            wall[p].append(progressive(f, acc, n_chunks, p, False)[0])
            kern[p].append(progressive(f, acc, n_chunks, p, True)[1])
        for (p, jp) in wall_jp:
            f.clear()
            wall_jp[(p, jp)].append(progressive(f, acc, n_chunks, p, False, job_pixels=jp)[0])
            if f.hash() != ref:
                print(f"passes={p} job_pixels={jp}: frame DIFFERS", file=sys.stderr)
                return False
    s_wall, s_kern = med([t[0] for t in single_t]), med([t[1] for t in single_t])
    out = {"frame": "scene_random_spheres t_cam1 1920x1080 1000 spp (250 chunks of 4) depth 50 f32", "sha256": ref, "frames_identical": True,
           "accumulator_MB": round(f.width * f.height * 64 / 1e6, 1),
           "single_render": {"wall_ms_median": s_wall, "wall_ms_min_max": spread([t[0] for t in single_t]), "kernel_ms_median": s_kern,
                             "kernel_ms_min_max": spread([t[1] for t in single_t])}, "rows": []}
    for p in rows:
        r = {"passes": p, "wall_ms_median": med(wall[p]), "wall_ms_min_max": spread(wall[p]), "kernel_ms_sum_median": med(kern[p]),
             "kernel_ms_sum_min_max": spread(kern[p]), "wall_vs_single": round(med(wall[p]) / s_wall, 4), "kernel_vs_single": round(med(kern[p]) / s_kern, 4)}
        if p in jp_rows:
            r["wall_ms_median_by_job_pixels"] = {str(jp): med(wall_jp[(p, jp)]) for jp in (1, 4, 16)}
        out["rows"].append(r)
        print(json.dumps(r), flush=True)
    if a.baseline_lib:
        env = dict(os.environ)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--single-only", "--lib", a.baseline_lib, "--reps", str(a.reps)],
                           capture_output=True, text=True, env=env, timeout=300)
        if r.returncode != 0:
            print("baseline library run failed:\n" + r.stderr[-2000:], file=sys.stderr)
            return False
        b = json.loads(r.stdout.strip().splitlines()[-1])
        if b["sha256"] != ref:
            print("the baseline library's frame differs", file=sys.stderr)
            return False
        out["baseline_library_single_render"] = {"wall_ms_median": med(b["wall_ms"]), "wall_ms_min_max": spread(b["wall_ms"]),
                                                 "kernel_ms_median": med(b["kernel_ms"]), "kernel_ms_min_max": spread(b["kernel_ms"]), "frame_identical": True}
        print("baseline", json.dumps(out["baseline_library_single_render"]), flush=True)
    print("single", json.dumps(out["single_render"]), flush=True)
    L.rtw_accum_free(acc)
    res["passes"] = out
    return True


def measure_interactive(L, a, res):
    res["interactive"] = {}
    ok = True
    for name, width, depth, n in (("320x180_d16", 320, 16, 256), ("1920x1080_d50", 1920, 50, 64)):
        f = Frame(L, width, 4096, depth, n_chunks=4096)           # 4096 chunks of 1 sample: nothing is paid for the ones not rendered
        acc = C.c_void_p()
        f.check(L.rtw_accum_create(0, f.width, f.height, C.byref(acc)))
        out = C.c_void_p(f.buf.data_ptr())

        def run(sync):
            f.check(L.rtw_accum_reset(acc, f.sp))
            f.stream.synchronize()
            kernel = 0.0
            t0 = time.perf_counter()
            for k in range(n):
                f.check(L.rtw_render_accum_f32(f.scene, C.byref(f.cam), C.byref(f.P), k, 1, acc, out, f.sp))
                if sync:
                    kernel += f.stats().kernel_ms
            f.stats()
            return time.perf_counter() - t0, kernel

        run(False)
        got = f.hash()
        one = Frame(L, width, n, depth, n_chunks=n)              # the prefix property: n passes of 1 sample = render(spp = n, n_chunks = n)
        one.single()
        same = got == one.hash()
        ok &= same
        print(f"interactive {name}: running image after {n} passes {'identical to' if same else 'DIFFERS from'} the {n}-spp render", flush=True)
        if not same:
            continue
        pipe = [run(False)[0] for _ in range(a.reps)]
        sync = [run(True) for _ in range(a.reps)]
        r = {"width": f.width, "height": f.height, "depth": depth, "passes_timed": n, "frame_identical": True,
             "pipelined_passes_per_s": round(n / statistics.median(pipe), 1), "pipelined_ms_per_pass": round(statistics.median(pipe) / n * 1e3, 4),
             "synchronous_passes_per_s": round(n / statistics.median([s[0] for s in sync]), 1),
             "synchronous_ms_per_pass": round(statistics.median([s[0] for s in sync]) / n * 1e3, 4),
             "kernel_ms_per_pass": round(statistics.median([s[1] for s in sync]) / n, 4)}
        res["interactive"][name] = r
        print(name, json.dumps(r), flush=True)
        L.rtw_accum_free(acc)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "progressive_frames.json"))
    ap.add_argument("--baseline-lib", default=None, help="another build of librtw_hip.so whose single render is timed in a child process")
    ap.add_argument("--only", default="passes,interactive")
    ap.add_argument("--single-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.single_only:
        return single_only(a)
    import torch                         # torch's HIP runtime first: the frames live in torch buffers
    torch.cuda.init()
    L = _capi.lib()
    res = {"tool": "tools/gpu_progressive.py", "reps": a.reps}
    ok = True
    if "passes" in a.only:
        ok &= measure_passes(L, a, res)
    if "interactive" in a.only:
        ok &= measure_interactive(L, a, res)
    if ok:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
