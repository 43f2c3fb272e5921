#!/usr/bin/env python3
"""What a batched adaptive render buys (include/rtw_hip.h rtw_render_adaptive_batch_*), on one MI355X.
usage: python tools/gpu_adaptive_batch.py [--reps 5] [--tolerances 0.1,0.03] [--out profiles/adaptive_batch_frames.json]

  gain      16 views of scene_random_spheres on a circle round t_cam1's look-at point (view 0 is t_cam1 itself), 480 x 270, 1000 spp
            (250 chunks of 4), depth 50, Float32, one seed per view: ONE rtw_render_adaptive_batch_f32 against 16 sequential
            rtw_render_adaptive_f32, fresh accumulators each time, the two alternating within a repetition.  Wall time (host clock around
            the blocking calls; median and min / max of --reps), the passes (= launches = host waits) of either side, the active tiles of
            every batched pass, and the summed HIP-event time of the trace kernels (rtw_stats).  The SHA-256 of every view's words is
            compared between the two FIRST; a mismatch fails the run.
  one_view  the headline frame (t_cam1, 1920 x 1080, 1000 spp, depth 50) as a batch of ONE view against the single call: the price of
            the view table.
  one_view_paths  where a batch of one loses: the same frame through each pair of entry points, summed trace-kernel time -- the one-shot
            render against rtw_render_batch_device_f32, one progressive pass of 32 chunks against rtw_render_accum_batch_f32, and the
            first pass of an adaptive render alone (a tolerance every tile meets at once) against rtw_render_adaptive_batch_f32.
  kernels   per tolerance ONE batched and ONE sequential run of the `gain` workload, each in a child process under `rocprofv3
            --kernel-trace --stats`: the summed device time and the launches of the trace kernels, the check kernels, the compaction
            (count / scan / scatter; and once more with the single call's one-workgroup loop, RTW_BATCH_COMPACT=loop) and the advance."""
import argparse
import ctypes as C
import hashlib
import json
import math
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rtw_amd as R                      # noqa: E402
from rtw_amd import _capi                # noqa: E402
from rtw_amd.adaptive import DEFAULT_DARK_FLOOR, checkpoints  # noqa: E402
from gpu_progressive import med, spread  # noqa: E402

N_CHUNKS = 250
T = np.float32


def circle_cameras(n):
    """n cameras like t_cam1 -- look-at (0, 0, 0), 20 degrees, aperture 0.1, focus 10 -- on the horizontal circle through t_cam1's position"""
    x0, y0, z0 = 13.0, 2.0, 3.0
    r, phi0 = math.hypot(x0, z0), math.atan2(z0, x0)
    cams = [R.t_cam1(elem_type=T)]
    for k in range(1, n):
        phi = phi0 + 2.0 * math.pi * k / n
        cams.append(R.default_camera((r * math.cos(phi), y0, r * math.sin(phi)), (0, 0, 0), (0, 1, 0), 20, 16 / 9, 0.1, 10.0, elem_type=T))
    return cams


class Views:
    """one uploaded scene, n cameras, two sets of n accumulators (batched / sequential) on device 0"""

    def __init__(self, L, cams, width, spp, depth):
        self.L, self.n = L, len(cams)
        self.width, self.height, self.spp, self.depth = width, R.image_height(width), spp, depth
        R.reseed()                                                # (the same 485 spheres every time)
        S, keep = _capi.make_scene(R.flatten_scene(R.scene_random_spheres(elem_type=T), T), T)
        self.scene = C.c_void_p()
        self.check(L.rtw_scene_upload_f32(C.byref(S), 0, C.byref(self.scene)))
        self.cams = _capi.make_cameras(cams, T)
        self.seeds = _capi.make_seeds([1 + v for v in range(self.n)], self.n)
        self.sets = []
        for _ in range(2):
            accs = []
            for _ in range(self.n):
                a = C.c_void_p()
                self.check(L.rtw_accum_create(0, self.width, self.height, C.byref(a)))
                accs.append(a)
            self.sets.append(accs)
        self.handles = _capi.make_handles(self.sets[0])
        self.n_tiles = ((self.height + 7) // 8) * ((self.width + 7) // 8)
        import torch
        self.stream = torch.cuda.Stream()
        self.sp = C.c_void_p(self.stream.cuda_stream)

    def check(self, rc):
        if rc:
            raise RuntimeError(f"librtw_hip error {rc}: {self.L.rtw_last_error().decode()}")

    def params(self, seed=1):
        return _capi.make_params(self.width, self.height, self.spp, self.depth, seed, 0)

    def reset(self, accs):
        for a in accs:
            self.check(self.L.rtw_accum_reset(a, self.sp))
        self.stream.synchronize()                                 # (the clearing is not part of what is timed)

    def stats(self):
        st = _capi.Stats()
        self.check(self.L.rtw_stats(C.byref(st)))
        return st

    def batched(self, tol):
        """-> (wall ms, summed trace-kernel ms)"""
        self.reset(self.sets[0])
        A = _capi.Adaptive(tol, DEFAULT_DARK_FLOOR, 0, 0)
        P = self.params()
        t0 = time.perf_counter()
        self.check(self.L.rtw_render_adaptive_batch_f32(self.scene, self.cams, self.n, self.seeds, C.byref(P), C.byref(A), self.handles, None, self.sp))
        wall = (time.perf_counter() - t0) * 1e3
        return wall, self.stats().kernel_ms

    def sequential(self, tol):
        """-> (wall ms, summed trace-kernel ms)"""
        self.reset(self.sets[1])
        A = _capi.Adaptive(tol, DEFAULT_DARK_FLOOR, 0, 0)
        Ps = [self.params(self.seeds[v]) for v in range(self.n)]
        kernel = 0.0
        t0 = time.perf_counter()
        for v in range(self.n):
            self.check(self.L.rtw_render_adaptive_f32(self.scene, C.byref(self.cams[v]), C.byref(Ps[v]), C.byref(A), self.sets[1][v], None, self.sp))
            kernel += self.stats().kernel_ms                     # (resolved by the blocking call: a read of the thread's record)
        wall = (time.perf_counter() - t0) * 1e3
        return wall, kernel

    def words_sha(self, a):
        out = np.empty(self.width * self.height * 8, np.uint64)
        self.check(self.L.rtw_accum_read_pixels(a, out.ctypes.data_as(C.c_void_p)))
        return hashlib.sha256(out.tobytes()).hexdigest()

    def chunks(self, a):
        buf = np.zeros(self.n_tiles, np.int32)
        n = C.c_int32()
        self.check(self.L.rtw_accum_tile_chunks(a, buf.size, C.byref(n), buf.ctypes.data_as(C.POINTER(C.c_int32))))
        return buf

    def rounds(self, a):
        st = _capi.AdaptiveInfo()
        self.check(self.L.rtw_accum_adaptive_info(a, C.byref(st)))
        return st.rounds, st.samples

    def close(self):
        for accs in self.sets:
            for a in accs:
                self.L.rtw_accum_free(a)
        self.L.rtw_scene_free(self.scene)


def compare(V, tol, reps, label):
    """identity first, then the alternating timings -> dict (None: the words differ)"""
    V.batched(tol)
    V.sequential(tol)
    sha_b = [V.words_sha(a) for a in V.sets[0]]
    sha_s = [V.words_sha(a) for a in V.sets[1]]
    same = sha_b == sha_s and all(np.array_equal(V.chunks(a), V.chunks(b)) for a, b in zip(*V.sets))
    if not same:
        print(f"{label}: the batched accumulators DIFFER from the sequential ones at tolerance {tol}", file=sys.stderr)
        return None
    ct = np.stack([V.chunks(a) for a in V.sets[0]])
    cuts = [0] + checkpoints(N_CHUNKS)
    rounds_seq = [V.rounds(a)[0] for a in V.sets[1]]
    assert rounds_seq == [V.rounds(a)[0] for a in V.sets[0]]
    samples = sum(V.rounds(a)[1] for a in V.sets[0])
    active = [int((ct > c).sum()) for c in cuts if (ct > c).any()]
    bt, bk, st, sk = [], [], [], []
    for _ in range(reps):
        w, k = V.batched(tol); bt.append(w); bk.append(k)
        w, k = V.sequential(tol); st.append(w); sk.append(k)
    row = {"tolerance": tol, "views": V.n, "words_identical": True, "words_sha256_view0": sha_b[0],
           "samples": samples, "samples_vs_uniform": round(samples / (V.n * V.width * V.height * V.spp), 4),
           "batched": {"wall_ms_median": med(bt), "wall_ms_min_max": spread(bt), "trace_kernel_ms_sum_median": med(bk),
                       "passes": len(active), "launches_and_host_waits": len(active), "active_tiles_per_pass": active},
           "sequential": {"wall_ms_median": med(st), "wall_ms_min_max": spread(st), "trace_kernel_ms_sum_median": med(sk),
                          "passes": sum(rounds_seq), "launches_and_host_waits": sum(rounds_seq), "passes_per_view": rounds_seq},
           "gain_wall": round(med(st) / med(bt), 4), "gain_trace_kernel": round(med(sk) / med(bk), 4)}
    print(label, json.dumps(row), flush=True)
    return row


def one_view_paths(V, reps):
    """V: ONE view.  -> rows of {path, single ms, batch-of-one ms, ratio} (summed trace-kernel time, median (min, max) of reps)"""
    import torch
    L, P, A = V.L, V.params(V.seeds[0]), _capi.Adaptive(1e9, DEFAULT_DARK_FLOOR, 0, 0)
    img = torch.empty(V.width * V.height * 3, dtype=torch.float32, device="cuda:0")
    out, acc, cam = C.c_void_p(img.data_ptr()), V.sets[0][0], C.byref(V.cams[0])

    def timed(call, fresh):
        if fresh:
            V.reset(V.sets[0])
        V.check(call())
        return V.stats().kernel_ms
    pairs = (("one-shot render", False, lambda: L.rtw_render_device_f32(V.scene, cam, C.byref(P), out, V.sp),
              lambda: L.rtw_render_batch_device_f32(V.scene, V.cams, 1, V.seeds, C.byref(P), out, V.sp)),
             ("progressive pass of 32 chunks", True, lambda: L.rtw_render_accum_f32(V.scene, cam, C.byref(P), 0, 32, acc, None, V.sp),
              lambda: L.rtw_render_accum_batch_f32(V.scene, V.cams, 1, V.seeds, C.byref(P), 0, 32, V.handles, None, V.sp)),
             ("adaptive render, first pass only (32 chunks)", True, lambda: L.rtw_render_adaptive_f32(V.scene, cam, C.byref(P), C.byref(A), acc, None, V.sp),
              lambda: L.rtw_render_adaptive_batch_f32(V.scene, V.cams, 1, V.seeds, C.byref(P), C.byref(A), V.handles, None, V.sp)))
    rows = []
    for name, fresh, single, batch in pairs:
        timed(single, fresh); timed(batch, fresh)
        s, b = [], []
        for _ in range(reps):
            s.append(timed(single, fresh)); b.append(timed(batch, fresh))
        row = {"path": name, "single_kernel_ms_median": med(s), "single_min_max": spread(s), "batch_of_one_kernel_ms_median": med(b),
               "batch_of_one_min_max": spread(b), "batch_of_one_vs_single": round(med(b) / med(s), 4)}
        print("one_view_paths", json.dumps(row), flush=True)
        rows.append(row)
    return rows


KERNEL_CLASSES = (("trace", "trace_kernel"), ("check", "accum_tile_check"), ("compaction", "accum_tile_compact"), ("compaction", "accum_tile_count"),
                  ("compaction", "accum_tile_scan"), ("compaction", "accum_tile_scatter"), ("advance", "accum_tile_advance"))


def traced(side, tol, views, loop=False):
    """one run of `side` in a child process under the profiler's kernel trace -> {class: {"us": summed device time, "launches": n}}"""
    env = dict(os.environ)
    if loop:
        env.update(RTW_ENABLE_TEST_AIDS="1", RTW_BATCH_COMPACT="loop")
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "t", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--child", side, "--tolerances", repr(tol), "--views", str(views)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            raise RuntimeError(f"kernel trace of {side} failed ({r.returncode}): {r.stderr[-400:]}")
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                for cls, key in KERNEL_CLASSES:
                    if key in row["Name"]:
                        c = out.setdefault(cls, {"us": 0.0, "launches": 0})
                        c["us"] = round(c["us"] + int(row["TotalDurationNs"]) / 1e3, 1)
                        c["launches"] += int(row["Calls"])
                        break
    return out


def child(a):
    """--child batched|sequential: ONE run of that side of the gain workload (what `traced` profiles)"""
    import torch
    torch.cuda.init()
    V = Views(_capi.lib(), circle_cameras(a.views), 480, 1000, 50)
    (V.batched if a.child == "batched" else V.sequential)(float(a.tolerances))
    V.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tolerances", default="0.1,0.03")
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_batch_frames.json"))
    ap.add_argument("--only", default="gain,one_view,one_view_paths,kernels")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    tols = [float(t) for t in a.tolerances.split(",")]
    import torch                         # torch's HIP runtime first
    torch.cuda.init()
    L = _capi.lib()
    res = {"tool": "tools/gpu_adaptive_batch.py", "reps": a.reps, "dark_floor": DEFAULT_DARK_FLOOR, "checkpoints": checkpoints(N_CHUNKS)}
    ok = True
    a.only = a.only.replace(" ", "")
    if "gain" in a.only.split(","):
        V = Views(L, circle_cameras(a.views), 480, 1000, 50)
        res["gain"] = {"frame": f"{a.views} views of scene_random_spheres round t_cam1's look-at point, 480x270, 1000 spp (250 chunks of 4), depth 50, f32", "rows": []}
        for tol in tols:
            row = compare(V, tol, a.reps, "gain")
            ok &= row is not None
            res["gain"]["rows"].append(row)
        V.close()
    if "one_view_paths" in a.only.split(","):
        V = Views(L, circle_cameras(1), 1920, 1000, 50)
        res["one_view_paths"] = {"frame": "scene_random_spheres t_cam1 1920x1080 1000 spp (250 chunks of 4) depth 50 f32", "rows": one_view_paths(V, a.reps)}
        V.close()
    if "one_view" in a.only.split(","):
        V = Views(L, circle_cameras(1), 1920, 1000, 50)
        res["one_view"] = {"frame": "scene_random_spheres t_cam1 1920x1080 1000 spp (250 chunks of 4) depth 50 f32, a batch of ONE view against the single call", "rows": []}
        for tol in tols:
            row = compare(V, tol, a.reps, "one_view")
            ok &= row is not None
            res["one_view"]["rows"].append(row)
        V.close()
    if "kernels" in a.only.split(","):
        res["kernels"] = {"what": "summed device time (us) and launches per kernel class of ONE run, from the profiler's kernel trace", "rows": []}
        for tol in tols:
            row = {"tolerance": tol, "batched": traced("batched", tol, a.views), "batched_compaction_by_one_workgroup_loop": traced("batched", tol, a.views, loop=True),
                   "sequential": traced("sequential", tol, a.views)}
            print("kernels", json.dumps(row), flush=True)
            res["kernels"]["rows"].append(row)
    if ok:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
