#!/usr/bin/env python3
"""The first-hit feature pass next to the beauty render of the same frame (include/rtw_hip.h rtw_render_features_device_* vs
rtw_render_device_*, same rtw_params, same library), on one MI355X.
usage: python tools/gpu_features.py [--reps 7] [--warmup 2] [--out profiles/features_frames.json]

Cases, all scene_random_spheres through t_cam1, device-resident on one stream:
  f32_1080p_256     1920 x 1080 Float32, 256 spp (256 chunks of 1: every primary ray of the image is a feature sample)
  f32_1080p_1000    1920 x 1080 Float32, 1000 spp (250 chunks of 4: every 4th)
  f32_480x270_256   480 x 270 Float32, 256 spp
  f64_480x270_256   480 x 270 Float64, 256 spp
Per case: the kernel's HIP-event time from rtw_stats() (kernel_ms) of --reps calls after --warmup -- the median and the spread (min, max) --
for the feature pass and for the beauty render, their ratio, and the rates that go with them: the feature kernel's closest-hit scans per
second next to the trace kernel's ray segments (= closest-hit scans) per second.  A feature pass under RTW_FLAG_SCAN_VALU is timed too."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                             # noqa: E402  (torch's HIP runtime first: INTEGRATION.md section 5)
import rtw_amd as R                      # noqa: E402
from rtw_amd import _capi                # noqa: E402


def run_case(name, T, width, spp, reps, warmup):
    L = _capi.lib()
    f64 = np.dtype(T) == np.float64
    height = R.image_height(width)
    R.reseed()                           # reseed!(): the same scene in every case (485 spheres in Float32)
    flat = R.flatten_scene(R.scene_random_spheres(elem_type=T), T)
    S, keep = _capi.make_scene(flat, T)
    cam = _capi.make_camera(R.t_cam1(elem_type=T), T)
    handle = C.c_void_p()
    _capi.check((L.rtw_scene_upload_f64 if f64 else L.rtw_scene_upload_f32)(C.byref(S), 0, C.byref(handle)))
    tdt = torch.float64 if f64 else torch.float32
    d_feat = torch.empty(width * height * 8, dtype=tdt, device="cuda:0")
    d_img = torch.empty(width * height * 3, dtype=tdt, device="cuda:0")
    stream = torch.cuda.Stream()
    f_feat = L.rtw_render_features_device_f64 if f64 else L.rtw_render_features_device_f32
    f_img = L.rtw_render_device_f64 if f64 else L.rtw_render_device_f32
    n_eff = -(-spp // -(-spp // min(spp, 256)))

    def stats():
        st = _capi.Stats()
        _capi.check(L.rtw_stats(C.byref(st)))
        return st

    def features(flags=0):
        P = _capi.make_params(width, height, spp, 16, 1, 0, flags=flags)
        _capi.check(f_feat(handle, C.byref(cam), C.byref(P), 0, n_eff, C.c_void_p(d_feat.data_ptr()), C.c_void_p(stream.cuda_stream)))
        return stats()

    def beauty():
        P = _capi.make_params(width, height, spp, 16, 1, 0)
        _capi.check(f_img(handle, C.byref(cam), C.byref(P), C.c_void_p(d_img.data_ptr()), C.c_void_p(stream.cuda_stream)))
        return stats()

    def timed(fn):
        for _ in range(warmup):
            fn()
        sts = [fn() for _ in range(reps)]
        ms = [s.kernel_ms for s in sts]
        return sts[-1], statistics.median(ms), min(ms), max(ms)

    st_f, f_med, f_min, f_max = timed(features)
    ref = d_feat.cpu().numpy().tobytes()
    st_v, v_med, v_min, v_max = timed(lambda: features(_capi.FLAG_SCAN_VALU))
    same = d_feat.cpu().numpy().tobytes() == ref
    st_b, b_med, b_min, b_max = timed(beauty)
    assert st_f.n_chunks == st_b.n_chunks == n_eff and st_f.segments == width * height * n_eff
    cov = d_feat.cpu().numpy().reshape(width, height, 8)[..., 7]
    r = {"width": width, "height": height, "spp": spp, "n_chunks": int(st_f.n_chunks), "dtype": np.dtype(T).name, "spheres": int(flat["n"]),
         "feature_scans": int(st_f.segments), "feature_ms_median": round(f_med, 4), "feature_ms_min_max": [round(f_min, 4), round(f_max, 4)],
         "feature_valu_ms_median": round(v_med, 4), "feature_valu_ms_min_max": [round(v_min, 4), round(v_max, 4)], "valu_bytes_identical": same,
         "feature_grid_blocks": int(st_f.grid_blocks),
         "beauty_segments": int(st_b.segments), "beauty_ms_median": round(b_med, 4), "beauty_ms_min_max": [round(b_min, 4), round(b_max, 4)],
         "feature_over_beauty": round(f_med / b_med, 4),
         "feature_gscans_s": round(st_f.segments / f_med * 1e-6, 3), "feature_valu_gscans_s": round(st_v.segments / v_med * 1e-6, 3),
         "beauty_gsegments_s": round(st_b.segments / b_med * 1e-6, 3),
         "mean_coverage": round(float(cov.mean()), 4), "nan_values": int(np.isnan(cov).sum())}
    L.rtw_scene_free(handle)
    del keep
    print(name, json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_frames.json"))
    ap.add_argument("--cases", default="f32_1080p_256,f32_1080p_1000,f32_480x270_256,f64_480x270_256")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("no GPU: nothing is measured here", file=sys.stderr)
        return 1
    torch.cuda.init()
    cases = {"f32_1080p_256": (np.float32, 1920, 256), "f32_1080p_1000": (np.float32, 1920, 1000),
             "f32_480x270_256": (np.float32, 480, 256), "f64_480x270_256": (np.float64, 480, 256)}
    res = {"tool": "tools/gpu_features.py", "reps": a.reps, "warmup": a.warmup, "time": "rtw_stats().kernel_ms (HIP events around the kernel)", "cases": {}}
    for name in a.cases.split(","):
        T, width, spp = cases[name]
        res["cases"][name] = run_case(name, T, width, spp, a.reps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0 if all(r["valu_bytes_identical"] and r["nan_values"] == 0 for r in res["cases"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
