#!/usr/bin/env python3
"""Batched render vs the same frames one call at a time (include/rtw_hip.h rtw_render_batch_*), on one MI355X.
usage: python tools/gpu_batch_frames.py [--reps 50] [--warmup 5] [--out profiles/batch_frames.json]

Cases (BASELINE configs[0] / [1] and the Float64 render(scene_random_spheres, t_cam1, 200, 32)):
  cfg0_x64        64 views of scene_2_spheres 96 x 54, 16 spp, depth 4, f32: host entry points (one rtw_render_batch_f32 vs 64 rtw_render_f32)
  cfg0_x64_device the same pair device-resident (rtw_render_batch_device_f32 vs 64 rtw_render_device_f32 on one stream)
  cfg1_x8         8 views of scene_random_spheres 320 x 180, 64 spp, depth 16, f32 (host entry points)
  cfg1_x8_cull    the same with RTW_FLAG_GROUP_CULL
  f64_x16         16 views of scene_random_spheres 200 x 112, 32 spp, depth 16, Float64, t_cam1 (host entry points)
The views differ in camera (four cameras in turn) and seed.  Time per call = the median over --reps calls after --warmup, wall clock
around calls that return when the frames are done (host entry points; device-resident: the calls, then rtw_stats(), which waits for
the last render of the stream).  Every view of the batch is checked against its single render (sha256 of the frame bytes) before
anything is timed.  Kernel times are NOT taken here: run the tool under `rocprofv3 --kernel-trace --stats` for those."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rtw_amd as R                      # noqa: E402
from rtw_amd import _capi                # noqa: E402


def cameras(T, n):
    base = [R.t_cam1(elem_type=T), R.t_cam2(elem_type=T), R.t_default_cam(elem_type=T), R.default_camera((0, 1, 1), elem_type=T)]
    return [base[v % len(base)] for v in range(n)]


class Case:
    def __init__(self, name, scene, T, width, spp, depth, n, flags=0, device=False):
        self.name, self.T, self.width, self.spp, self.depth, self.n, self.flags, self.device = name, T, width, spp, depth, n, flags, device
        self.height = R.image_height(width)
        self.L = _capi.lib()
        self.flat = R.flatten_scene(scene, T)
        self.S, self.keep = _capi.make_scene(self.flat, T)
        self.cams = cameras(T, n)
        self.seeds = [1 + 7 * v for v in range(n)]
        self.cam_structs = [_capi.make_camera(c, T) for c in self.cams]
        self.cam_arr = _capi.make_cameras(self.cams, T)
        self.seed_arr = _capi.make_seeds(self.seeds, n)
        self.P = [_capi.make_params(width, self.height, spp, depth, s, 0, flags=flags) for s in self.seeds]
        self.frame = width * self.height * 3
        self.out = np.empty(n * self.frame, T)
        f64 = np.dtype(T) == np.float64
        L = self.L
        self.f_single = L.rtw_render_f64 if f64 else L.rtw_render_f32
        self.f_batch = L.rtw_render_batch_f64 if f64 else L.rtw_render_batch_f32
        if device:
            import torch
            self.handle = C.c_void_p()
            up = L.rtw_scene_upload_f64 if f64 else L.rtw_scene_upload_f32
            _capi.check(up(C.byref(self.S), 0, C.byref(self.handle)))
            self.buf = torch.empty(n * self.frame, dtype=torch.float64 if f64 else torch.float32, device="cuda:0")
            self.stream = torch.cuda.Stream()
            self.f_single_d = L.rtw_render_device_f64 if f64 else L.rtw_render_device_f32
            self.f_batch_d = L.rtw_render_batch_device_f64 if f64 else L.rtw_render_batch_device_f32

    def _wait(self):
        st = _capi.Stats()
        _capi.check(self.L.rtw_stats(C.byref(st)))
        return st

    def sequential(self):
        if self.device:
            base = self.buf.data_ptr()
            esz = self.buf.element_size()
            for v in range(self.n):
                _capi.check(self.f_single_d(self.handle, C.byref(self.cam_structs[v]), C.byref(self.P[v]), C.c_void_p(base + v * self.frame * esz),
                                            C.c_void_p(self.stream.cuda_stream)))
            return self._wait()
        for v in range(self.n):
            o = self.out[v * self.frame:(v + 1) * self.frame]
            _capi.check(self.f_single(C.byref(self.S), C.byref(self.cam_structs[v]), C.byref(self.P[v]), o.ctypes.data_as(C.c_void_p)))
        return self._wait()

    def batched(self):
        if self.device:
            _capi.check(self.f_batch_d(self.handle, self.cam_arr, self.n, self.seed_arr, C.byref(self.P[0]), C.c_void_p(self.buf.data_ptr()),
                                       C.c_void_p(self.stream.cuda_stream)))
            return self._wait()
        _capi.check(self.f_batch(C.byref(self.S), self.cam_arr, self.n, self.seed_arr, C.byref(self.P[0]), self.out.ctypes.data_as(C.c_void_p)))
        return self._wait()

    def hashes(self):
        data = self.buf.cpu().numpy() if self.device else self.out
        return [hashlib.sha256(data[v * self.frame:(v + 1) * self.frame].tobytes()).hexdigest() for v in range(self.n)]

    def close(self):
        if self.device:
            self.L.rtw_scene_free(self.handle)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_frames.json"))
    ap.add_argument("--cases", default="cfg0_x64,cfg0_x64_device,cfg1_x8,cfg1_x8_cull,f64_x16")
    a = ap.parse_args()
    f32, f64 = np.float32, np.float64
    make = {
        "cfg0_x64": lambda: Case("cfg0_x64", R.scene_2_spheres(elem_type=f32), f32, 96, 16, 4, 64),
        "cfg0_x64_device": lambda: Case("cfg0_x64_device", R.scene_2_spheres(elem_type=f32), f32, 96, 16, 4, 64, device=True),
        "cfg1_x8": lambda: Case("cfg1_x8", R.scene_random_spheres(elem_type=f32), f32, 320, 64, 16, 8),
        "cfg1_x8_cull": lambda: Case("cfg1_x8_cull", R.scene_random_spheres(elem_type=f32), f32, 320, 64, 16, 8, flags=_capi.FLAG_GROUP_CULL),
        "f64_x16": lambda: Case("f64_x16", R.scene_random_spheres(elem_type=f64), f64, 200, 32, 16, 16),
    }
    res = {"tool": "tools/gpu_batch_frames.py", "reps": a.reps, "warmup": a.warmup, "cases": {}}
    if any(n.endswith("_device") for n in a.cases.split(",")):
        import torch                     # torch's HIP runtime first: the device cases hand it torch buffers
        torch.cuda.init()
    for name in a.cases.split(","):
        c = make[name]()
        st_seq = c.sequential()
        h_seq = c.hashes()
        seg_seq = 0
        for v in range(c.n):                                      # (the single renders' segment counts, one call each)
            if c.device:
                _capi.check(c.f_single_d(c.handle, C.byref(c.cam_structs[v]), C.byref(c.P[v]), C.c_void_p(c.buf.data_ptr()), C.c_void_p(c.stream.cuda_stream)))
            else:
                o = c.out[:c.frame]
                _capi.check(c.f_single(C.byref(c.S), C.byref(c.cam_structs[v]), C.byref(c.P[v]), o.ctypes.data_as(C.c_void_p)))
            seg_seq += c._wait().segments
        st_b = c.batched()
        h_b = c.hashes()
        ok = h_b == h_seq and st_b.segments == seg_seq and st_b.samples == c.n * c.width * c.height * c.spp
        t_seq = timed(c.sequential, a.reps, a.warmup)
        t_b = timed(c.batched, a.reps, a.warmup)
        samples = c.n * c.width * c.height * c.spp
        m_seq, m_b = statistics.median(t_seq), statistics.median(t_b)
        r = {"views": c.n, "width": c.width, "height": c.height, "spp": c.spp, "depth": c.depth, "dtype": np.dtype(c.T).name,
             "group_cull": bool(c.flags & _capi.FLAG_GROUP_CULL), "device_resident": c.device, "frames_identical": ok,
             "segments": int(st_b.segments), "grid_blocks_batch": int(st_b.grid_blocks),
             "sequential_us_median": round(m_seq, 1), "sequential_us_p10_p90": [round(float(np.percentile(t_seq, 10)), 1), round(float(np.percentile(t_seq, 90)), 1)],
             "batch_us_median": round(m_b, 1), "batch_us_p10_p90": [round(float(np.percentile(t_b, 10)), 1), round(float(np.percentile(t_b, 90)), 1)],
             "sequential_msamples_s": round(samples / m_seq, 1), "batch_msamples_s": round(samples / m_b, 1), "speedup": round(m_seq / m_b, 2)}
        res["cases"][name] = r
        print(name, json.dumps(r), flush=True)
        c.close()
        if not ok:
            print(f"{name}: batch frames differ from the sequential renders", file=sys.stderr)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0 if all(r["frames_identical"] for r in res["cases"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
