#!/usr/bin/env python3
"""Batched feature + filter passes vs the loop of single-view calls (include/rtw_hip.h rtw_render_features_batch_*, rtw_filter_batch_*), on
one MI355X.
usage: python tools/gpu_filter_batch.py [--parent-lib PATH] [--out profiles/filter_batch_frames.json]

Shapes: 64 views of 96 x 54 and 16 views of 480 x 270, scene_random_spheres, 4 spp, depth 16, Float32, levels = 3, four cameras in turn,
a seed per view.  Everything is device-resident (torch buffers, one torch stream); a time is the span between two HIP events recorded on
that stream around the enqueued calls, the median of 25 after 5 warm-ups; the forms alternate inside every repetition.  Per shape:
  loop   (a) N x (rtw_render_features_device + rtw_denoise_device): N x (1 + 1 + levels) kernel launches
  batch  (b) rtw_render_features_batch_device + rtw_filter_batch_device: 1 + 1 + levels kernel launches
each alone ("feature+filter") and behind the one batched render of the N linear images ("pipeline").  The batch's outputs are compared with
the loop's, byte for byte, before anything is timed.
--parent-lib: a librtw_hip.so built from the PARENT commit.  The loop is then measured on it too, in a fresh child process started
before this one touches the GPU (the same card, the same call), and the ratio that decides is batch (this library) / loop (parent)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rtw_amd as R                      # noqa: E402
from rtw_amd import _capi                # noqa: E402

REPS, WARMUP, LEVELS, SPP, DEPTH = 25, 5, 3, 4, 16
SHAPES = {"64x96x54": (64, 96), "16x480x270": (16, 480)}
T = np.float32


def load(path, with_batch):
    """the library by its path, with the argument types of what this tool calls (a parent build has no batched passes)"""
    L = C.CDLL(path)
    L.rtw_last_error.restype = C.c_char_p
    cam, par, dn, vp, i32 = C.POINTER(_capi.CameraF32), C.POINTER(_capi.Params), C.POINTER(_capi.Denoise), C.c_void_p, C.c_int32
    L.rtw_scene_upload_f32.argtypes = [C.POINTER(_capi.SceneF32), C.c_int, C.POINTER(vp)]
    L.rtw_scene_free.argtypes = [vp]
    L.rtw_render_batch_device_f32.argtypes = [vp, cam, i32, C.POINTER(C.c_uint64), par, vp, vp]
    L.rtw_render_features_device_f32.argtypes = [vp, cam, par, i32, i32, vp, vp]
    L.rtw_denoise_device_f32.argtypes = [dn, i32, i32, vp, vp, vp, vp, vp]
    L.rtw_denoise_work_bytes.argtypes = [i32, i32, i32]
    L.rtw_denoise_work_bytes.restype = C.c_int64
    if with_batch:
        L.rtw_render_features_batch_device_f32.argtypes = [vp, cam, i32, C.POINTER(C.c_uint64), par, i32, i32, vp, vp]
        L.rtw_filter_batch_device_f32.argtypes = [dn, i32, i32, i32, vp, vp, vp, vp, vp]
    return L


def check(L, rc):
    if rc != 0:
        raise RuntimeError(f"librtw_hip error {rc}: {L.rtw_last_error().decode('utf-8', 'replace')}")


class Shape:
    def __init__(self, L, n, width, torch):
        self.L, self.n, self.W, self.H, self.torch = L, n, width, R.image_height(width), torch
        base = [R.t_cam1(elem_type=T), R.t_cam2(elem_type=T), R.t_default_cam(elem_type=T), R.default_camera((0, 1, 1), elem_type=T)]
        cams = [base[v % 4] for v in range(n)]
        self.seeds = [1 + 7 * v for v in range(n)]
        self.cam_structs = [_capi.make_camera(c, T) for c in cams]
        self.cam_arr, self.seed_arr = _capi.make_cameras(cams, T), _capi.make_seeds(self.seeds, n)
        R.reseed()
        S, self.keep = _capi.make_scene(R.flatten_scene(R.scene_random_spheres(elem_type=T), T), T)
        self.handle = C.c_void_p()
        check(L, L.rtw_scene_upload_f32(C.byref(S), 0, C.byref(self.handle)))
        self.P = [_capi.make_params(width, self.H, SPP, DEPTH, s, 0, gamma=0) for s in self.seeds]
        self.D = _capi.Denoise(LEVELS, 1, _capi.DENOISE_DEMODULATE, 1, -1, 0, 0.5, 0.1)
        self.pix = self.W * self.H
        new = lambda k: torch.empty(k, dtype=torch.float32, device="cuda:0")
        self.img, self.feat, self.out = new(n * self.pix * 3), new(n * self.pix * 8), new(n * self.pix * 3)
        self.work_one = int(L.rtw_denoise_work_bytes(self.W, self.H, 4))
        self.work = new(n * self.work_one // 4)
        self.stream = torch.cuda.Stream()
        self.s = C.c_void_p(self.stream.cuda_stream)
        torch.cuda.synchronize()

    def render(self):
        check(self.L, self.L.rtw_render_batch_device_f32(self.handle, self.cam_arr, self.n, self.seed_arr, C.byref(self.P[0]), C.c_void_p(self.img.data_ptr()), self.s))

    def loop(self):
        L, px = self.L, self.pix * 4
        for v in range(self.n):
            feat = C.c_void_p(self.feat.data_ptr() + v * px * 8)
            check(L, L.rtw_render_features_device_f32(self.handle, C.byref(self.cam_structs[v]), C.byref(self.P[v]), 0, SPP, feat, self.s))
            check(L, L.rtw_denoise_device_f32(C.byref(self.D), self.W, self.H, C.c_void_p(self.img.data_ptr() + v * px * 3), feat,
                                              C.c_void_p(self.out.data_ptr() + v * px * 3), C.c_void_p(self.work.data_ptr()), self.s))

    def batch(self):
        L = self.L
        check(L, L.rtw_render_features_batch_device_f32(self.handle, self.cam_arr, self.n, self.seed_arr, C.byref(self.P[0]), 0, SPP, C.c_void_p(self.feat.data_ptr()), self.s))
        check(L, L.rtw_filter_batch_device_f32(C.byref(self.D), self.W, self.H, self.n, C.c_void_p(self.img.data_ptr()), C.c_void_p(self.feat.data_ptr()),
                                               C.c_void_p(self.out.data_ptr()), C.c_void_p(self.work.data_ptr()), self.s))

    def span_ms(self, *steps):
        e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        e0.record(self.stream)
        for step in steps:
            step()
        e1.record(self.stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def fetch(self):
        self.stream.synchronize()
        return self.out.cpu().numpy().tobytes(), self.feat.cpu().numpy().tobytes()

    def close(self):
        self.stream.synchronize()
        self.L.rtw_scene_free(self.handle)


def med(xs):
    return {"ms_median": round(statistics.median(xs), 4), "ms_p10_p90": [round(float(np.percentile(xs, 10)), 4), round(float(np.percentile(xs, 90)), 4)]}


def measure(lib_path, with_batch):
    import torch                     # torch's HIP runtime first: the calls get torch buffers and a torch stream
    torch.cuda.init()
    L = load(lib_path, with_batch)
    res = {}
    for name, (n, width) in SHAPES.items():
        sh = Shape(L, n, width, torch)
        sh.render()
        forms = {"loop": sh.loop}
        r = {"views": n, "width": sh.W, "height": sh.H, "spp": SPP, "levels": LEVELS, "kernel_launches": {"render": 1, "loop": n * (2 + LEVELS)}}
        if with_batch:
            forms["batch"] = sh.batch
            r["kernel_launches"]["batch"] = 2 + LEVELS
            sh.loop()
            ref = sh.fetch()
            sh.out.fill_(-7.0)
            sh.feat.fill_(-7.0)
            torch.cuda.synchronize()
            sh.batch()
            r["outputs_identical"] = sh.fetch() == ref
        times = {f"{k}_{part}": [] for k in forms for part in ("feature_filter", "pipeline")}
        for rep in range(WARMUP + REPS):
            for k, fn in forms.items():                      # (the forms alternate inside a repetition)
                a, b = sh.span_ms(fn), sh.span_ms(sh.render, fn)
                if rep >= WARMUP:
                    times[f"{k}_feature_filter"].append(a)
                    times[f"{k}_pipeline"].append(b)
        r.update({k: med(v) for k, v in times.items()})
        res[name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
        sh.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="librtw_hip.so of the parent commit: its loop is measured too, in a child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_batch_frames.json"))
    ap.add_argument("--loop-only", metavar="LIB", default=None, help="(the child of --parent-lib) measure the loop on LIB, print JSON")
    a = ap.parse_args()
    if a.loop_only:
        print(json.dumps(measure(a.loop_only, False)))
        return 0
    res = {"tool": "tools/gpu_filter_batch.py", "reps": REPS, "warmup": WARMUP, "dtype": "float32", "scene": "scene_random_spheres", "depth": DEPTH,
           "timing": "HIP events on the calls' stream around the enqueued calls, median; device-resident buffers"}
    parent = None
    if a.parent_lib:                       # (before this process initialises the GPU)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop-only", os.path.abspath(a.parent_lib)], capture_output=True, text=True, check=True, timeout=900)
        parent = json.loads(out.stdout.strip().splitlines()[-1])
    res["shapes"] = measure(_capi.LIB_PATH, True)
    for name, r in res["shapes"].items():
        r["ratio_batch_over_loop"] = {part: round(r[f"batch_{part}"]["ms_median"] / r[f"loop_{part}"]["ms_median"], 4) for part in ("feature_filter", "pipeline")}
        if parent:
            r["parent_loop_feature_filter"], r["parent_loop_pipeline"] = parent[name]["loop_feature_filter"], parent[name]["loop_pipeline"]
            r["ratio_batch_over_parent_loop"] = {part: round(r[f"batch_{part}"]["ms_median"] / parent[name][f"loop_{part}"]["ms_median"], 4)
                                                 for part in ("feature_filter", "pipeline")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: (r.get("ratio_batch_over_parent_loop") or r["ratio_batch_over_loop"]) for k, r in res["shapes"].items()}))
    return 0 if all(r["outputs_identical"] for r in res["shapes"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
