#!/usr/bin/env python3
"""The batched one call over accumulators vs the per-view loop (include/rtw_hip.h rtw_accum_filtered_batch_* vs rtw_accum_filtered_*), on one
MI355X.
usage: python tools/gpu_accum_filter_batch.py [--out profiles/accum_filter_batch_frames.json]

Shapes: 16 views of 96 x 54 and 16 views of 480 x 270 (the frames of DESIGN.md 7.8 and 7.12), scene_random_spheres, at most 64 spp in 64
chunks, depth 16, Float32, four cameras in turn, a seed per view; the accumulators are filled ONCE by rtw_render_adaptive_batch_* (tolerance
0.05, dark_floor 0.03, checkpoints every 16 chunks) and only read afterwards.  levels = 3, guided.  Per shape:
  loop   N x rtw_accum_filtered_f32: N x (resolve + tiled feature pass + noise map + prepare + levels) launches, N blocking D2H -- the path
         before the batched forms existed; it is unchanged, so it is the reference
  batch  rtw_accum_filtered_batch_f32: 4 + levels launches, one D2H
Both forms block until their result is in host memory, so a time is the span between two HIP events recorded on one stream before and after
the whole sequence (the second is recorded when the host returns from the last call); the median of 25 after 5 warm-ups, the forms
alternating inside every repetition.  The batch's frames are compared with the loop's, byte for byte, before anything is timed.  The pure
device-side share of the batch is measured too: the four device-resident calls (rtw_accum_resolve_batch_*, _features_batch_*, _noise_batch_*,
rtw_guided_filter_batch_device_*) enqueued on one stream between two events, against the same loop of the single device-resident calls."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rtw_amd as R                      # noqa: E402
from rtw_amd import _capi                # noqa: E402

REPS, WARMUP, LEVELS, SPP, DEPTH, TOL, FLOOR, CHECK = 25, 5, 3, 64, 16, 0.05, 0.03, 16
SHAPES = {"16x96x54": (16, 96), "16x480x270": (16, 480)}
T = np.float32


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
        _capi.check(L.rtw_scene_upload_f32(C.byref(S), 0, C.byref(self.handle)))
        self.accs = []
        for _ in range(n):
            a = C.c_void_p()
            _capi.check(L.rtw_accum_create(0, width, self.H, C.byref(a)))
            self.accs.append(a)
        self.acc_arr = _capi.make_handles(self.accs)
        self.P = [_capi.make_params(width, self.H, SPP, DEPTH, s, SPP, gamma=1) for s in self.seeds]
        A = _capi.Adaptive(TOL, FLOOR, CHECK, CHECK)
        _capi.check(L.rtw_render_adaptive_batch_f32(self.handle, self.cam_arr, n, self.seed_arr, C.byref(self.P[0]), C.byref(A), self.acc_arr, None, None))
        self.held = 0
        for a in self.accs:
            st = _capi.AdaptiveInfo()
            _capi.check(L.rtw_accum_adaptive_info(a, C.byref(st)))
            self.held += st.samples
        self.D = _capi.Denoise(LEVELS, 1, _capi.DENOISE_DEMODULATE, 1, -1, 0, 1.0, 0.1)
        self.pix = self.W * self.H
        self.out_loop, self.out_batch = np.zeros(n * self.pix * 3, T), np.zeros(n * self.pix * 3, T)
        new = lambda k: torch.empty(k, dtype=torch.float32, device="cuda:0")
        self.img, self.feat, self.noise, self.out = new(n * self.pix * 3), new(n * self.pix * 8), new(n * self.pix), new(n * self.pix * 3)
        self.work = new(n * int(L.rtw_denoise_work_bytes(self.W, self.H, 4)) // 4)
        self.stream = torch.cuda.Stream()
        self.s = C.c_void_p(self.stream.cuda_stream)
        torch.cuda.synchronize()

    # ---- the host forms: blocking, the result in host memory ----
    def loop(self):
        L, e = self.L, self.pix * 3
        for v in range(self.n):
            _capi.check(L.rtw_accum_filtered_f32(self.handle, C.byref(self.cam_structs[v]), C.byref(self.P[v]), C.byref(self.D), self.accs[v], 1,
                                                 self.out_loop[v * e:].ctypes.data_as(C.c_void_p)))

    def batch(self):
        _capi.check(self.L.rtw_accum_filtered_batch_f32(self.handle, self.cam_arr, self.n, self.seed_arr, C.byref(self.P[0]), C.byref(self.D), self.acc_arr, 1,
                                                        self.out_batch.ctypes.data_as(C.c_void_p)))

    # ---- the device-resident forms: asynchronous on self.stream ----
    def loop_device(self):
        L, px = self.L, self.pix * 4
        for v in range(self.n):
            img, feat = C.c_void_p(self.img.data_ptr() + v * px * 3), C.c_void_p(self.feat.data_ptr() + v * px * 8)
            noise = C.c_void_p(self.noise.data_ptr() + v * px)
            _capi.check(L.rtw_accum_resolve_f32(self.accs[v], 0, img, self.s))
            _capi.check(L.rtw_accum_features_f32(self.handle, C.byref(self.cam_structs[v]), C.byref(self.P[v]), self.accs[v], feat, self.s))
            _capi.check(L.rtw_accum_noise_f32(self.accs[v], noise, self.s))
            _capi.check(L.rtw_guided_filter_device_f32(C.byref(self.D), self.W, self.H, img, feat, noise, C.c_void_p(self.out.data_ptr() + v * px * 3),
                                                       C.c_void_p(self.work.data_ptr()), self.s))

    def batch_device(self):
        L, p = self.L, lambda t: C.c_void_p(t.data_ptr())
        _capi.check(L.rtw_accum_resolve_batch_f32(self.acc_arr, self.n, 0, p(self.img), self.s))
        _capi.check(L.rtw_accum_features_batch_f32(self.handle, self.cam_arr, self.n, self.seed_arr, C.byref(self.P[0]), self.acc_arr, p(self.feat), self.s))
        _capi.check(L.rtw_accum_noise_batch_f32(self.acc_arr, self.n, p(self.noise), self.s))
        _capi.check(L.rtw_guided_filter_batch_device_f32(C.byref(self.D), self.W, self.H, self.n, p(self.img), p(self.feat), p(self.noise), p(self.out), p(self.work), self.s))

    def span_ms(self, step):
        e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        e0.record(self.stream)
        step()
        e1.record(self.stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def fetch_device(self):
        self.stream.synchronize()
        return self.out.cpu().numpy().tobytes()

    def close(self):
        self.stream.synchronize()
        for a in self.accs:
            self.L.rtw_accum_free(a)
        self.L.rtw_scene_free(self.handle)


def med(xs):
    return {"ms_median": round(statistics.median(xs), 4), "ms_p10_p90": [round(float(np.percentile(xs, 10)), 4), round(float(np.percentile(xs, 90)), 4)]}


def measure():
    import torch                     # torch's HIP runtime first
    torch.cuda.init()
    L = _capi.lib()
    res = {}
    for name, (n, width) in SHAPES.items():
        sh = Shape(L, n, width, torch)
        per_view = 3 + 1 + LEVELS
        r = {"views": n, "width": sh.W, "height": sh.H, "max_spp": SPP, "tolerance": TOL, "samples_held_per_pixel": round(sh.held / (n * sh.pix), 3), "levels": LEVELS,
             "guided": 1, "kernel_launches": {"loop": n * per_view, "batch": per_view}, "d2h": {"loop": n, "batch": 1}}
        sh.loop()
        sh.batch()
        r["outputs_identical"] = sh.out_loop.tobytes() == sh.out_batch.tobytes()
        sh.loop_device()
        ref = sh.fetch_device()
        sh.out.fill_(-7.0)
        torch.cuda.synchronize()
        sh.batch_device()
        r["device_outputs_identical"] = sh.fetch_device() == ref and ref == sh.out_loop.tobytes()
        forms = {"loop": sh.loop, "batch": sh.batch, "loop_device": sh.loop_device, "batch_device": sh.batch_device}
        times = {k: [] for k in forms}
        for rep in range(WARMUP + REPS):
            for k, fn in forms.items():                      # (the forms alternate inside a repetition)
                t = sh.span_ms(fn)
                if rep >= WARMUP:
                    times[k].append(t)
        r.update({k: med(v) for k, v in times.items()})
        r["ratio_batch_over_loop"] = {"one_call": round(r["batch"]["ms_median"] / r["loop"]["ms_median"], 4),
                                      "device_resident": round(r["batch_device"]["ms_median"] / r["loop_device"]["ms_median"], 4)}
        res[name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
        sh.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_filter_batch_frames.json"))
    a = ap.parse_args()
    res = {"tool": "tools/gpu_accum_filter_batch.py", "reps": REPS, "warmup": WARMUP, "dtype": "float32", "scene": "scene_random_spheres", "depth": DEPTH,
           "timing": "HIP events on one stream before and after the whole sequence, median; one_call: blocking host forms (result in host memory), "
                     "device_resident: the asynchronous calls on that stream",
           "shapes": measure()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: r["ratio_batch_over_loop"] for k, r in res["shapes"].items()}))
    return 0 if all(r["outputs_identical"] and r["device_outputs_identical"] for r in res["shapes"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
