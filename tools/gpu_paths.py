#!/usr/bin/env python3
"""Batched temporal steps on the GPU: what one launch for S paths saves against S launches.

    python tools/gpu_paths.py [--out profiles/paths_frames.json] [--repeats 30]

step     one batched step (rtw_reproject_batch_device_f32) against S single steps (rtw_temporal_device_f32 / rtw_clamped_step_device_f32)
         enqueued on ONE stream, S in {2, 16}, at 96x54, 480x270 and 1920x1080, Float32, plain and clamped (radius 1, no guides), on synthetic
         frames (a surface at depth 4 with a noisy image) and the states a first-frame step left.  Time: HIP events around the enqueued work,
         per repeat; the two variants ALTERNATE inside one process (A B A B ...), after a warm-up, so drift hits both alike.
call     rtw_render_paths_f32 (render_sequences) against S calls of rtw_render_path_clamped_f32 (render_sequence(clamp=True)), same S, at
         the two small sizes, 8 steps, 1 spp, two-sphere scene: wall clock around the blocking calls, alternating.
control  the batched step at S = 1 against the single step at 1920x1080: what the table's loads and the path arithmetic cost.
Every entry reports the median and the spread (min, max, inter-quartile range) over the repeats, in milliseconds.  Nothing here is a gate."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    q1, q3 = np.percentile(a, [25, 75])
    return dict(median_ms=round(float(np.median(a)), 5), min_ms=round(float(a[0]), 5), max_ms=round(float(a[-1]), 5), iqr_ms=round(float(q3 - q1), 5), repeats=len(a))


def orbit(R, S, k, T=np.float32):
    return [R.default_camera(lookfrom=(1.5 * np.sin(0.03 * k) + 0.065 * s, 0.4, -1 + 1.5 * np.cos(0.03 * k)), lookat=(0, 0, -1), vfov=60, aperture=0, elem_type=T) for s in range(S)]


def step_entry(R, torch, W, H, S, clamp, repeats):
    T, n = np.float32, W * H
    rng = np.random.default_rng(7)
    img = torch.from_numpy(rng.uniform(0.1, 0.9, S * n * 3).astype(T)).cuda()
    f = np.zeros((S * n, 8), T)
    f[:, 0:3], f[:, 5], f[:, 6], f[:, 7] = 0.5, 1.0, 4.0, 1.0          # albedo, normal (0, 0, 1), depth 4, coverage 1
    feat = torch.from_numpy(f.reshape(-1)).cuda()
    ns = R.temporal_state_bytes(W, H, T) // 4
    st = [torch.zeros(S * ns, dtype=torch.float32, device="cuda:0") for _ in range(2)]
    out = torch.zeros(S * n * 3, dtype=torch.float32, device="cuda:0")
    c0, c1 = orbit(R, S, 0), orbit(R, S, 1)
    tab = torch.from_numpy(R.temporal_path_table(c1, c0).reshape(-1)).cuda()
    tab0 = torch.from_numpy(R.temporal_path_table(c0).reshape(-1)).cuda()
    torch.cuda.synchronize()
    R.temporal_step_batch_into(out.data_ptr(), st[0].data_ptr(), img.data_ptr(), feat.data_ptr(), tab0.data_ptr(), S, W, H)      # the previous states
    ck = dict(radius=1, guides=False, sigma=1.0, len_scale=1.0) if clamp else None

    def batched():
        R.temporal_step_batch_into(out.data_ptr(), st[1].data_ptr(), img.data_ptr(), feat.data_ptr(), tab.data_ptr(), S, W, H, clamp=ck, d_states_prev_ptr=st[0].data_ptr())

    def singles():
        for s in range(S):
            o, a, b = out[s * n * 3:].data_ptr(), st[1][s * ns:].data_ptr(), st[0][s * ns:].data_ptr()
            i, g = img[s * n * 3:].data_ptr(), feat[s * n * 8:].data_ptr()
            if clamp:
                R.temporal_step_clamped_into(o, a, i, g, c1[s], W, H, clamp=ck, d_state_prev_ptr=b, cam_prev=c0[s])
            else:
                R.temporal_step_into(o, a, i, g, c1[s], W, H, d_state_prev_ptr=b, cam_prev=c0[s])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(5):
        timed(batched), timed(singles)
    a, b = [], []
    for _ in range(repeats):
        a.append(timed(batched))
        b.append(timed(singles))
    return dict(width=W, height=H, paths=S, step="clamped" if clamp else "plain", batched=stats(a), singles=stats(b),
                ratio_singles_over_batched=round(float(np.median(b) / np.median(a)), 3))


def call_entry(R, W, S, repeats, steps=8):
    T = np.float32
    scene = R.scene_2_spheres(elem_type=T)
    paths = [[orbit(R, S, k)[s] for k in range(steps)] for s in range(S)]
    seeds = [[1 + 100 * s + k for k in range(steps)] for s in range(S)]

    def batched():
        R.render_sequences(scene, paths, W, 1, seeds=seeds, clamp=True)

    def singles():
        for s in range(S):
            R.render_sequence(scene, paths[s], W, 1, seeds=seeds[s], clamp=True)

    def timed(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    for _ in range(3):
        timed(batched), timed(singles)
    a, b = [], []
    for _ in range(repeats):
        a.append(timed(batched))
        b.append(timed(singles))
    return dict(width=W, height=W * 9 // 16, paths=S, steps=steps, spp=1, paths_call=stats(a), sequence_calls=stats(b),
                ratio_calls_over_paths_call=round(float(np.median(b) / np.median(a)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paths_frames.json"))
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    import torch
    import rtw_amd as R
    res = dict(device=torch.cuda.get_device_name(0), elem_type="float32",
               time="step / control: HIP events around the enqueued launches on one stream; call: wall clock around the blocking calls; the two variants alternate in "
                    "one process after a warm-up; median, min, max and inter-quartile range over the repeats",
               step=[], call=[], control=[])
    for W, H in ((96, 54), (480, 270), (1920, 1080)):
        for S in (2, 16):
            for clamp in (False, True):
                res["step"].append(step_entry(R, torch, W, H, S, clamp, args.repeats))
                print(json.dumps(res["step"][-1]), flush=True)
    for W in (96, 480):
        for S in (2, 16):
            res["call"].append(call_entry(R, W, S, max(5, args.repeats // 3)))
            print(json.dumps(res["call"][-1]), flush=True)
    for clamp in (False, True):
        res["control"].append(step_entry(R, torch, 1920, 1080, 1, clamp, args.repeats))
        print(json.dumps(res["control"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
