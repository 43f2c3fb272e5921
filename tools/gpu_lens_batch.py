#!/usr/bin/env python3
"""The batched lens stages on one MI355X (include/rtw_hip.h rtw_lens_batch_device_*): the measurements of DESIGN.md 7.28, written to
profiles/lens_batch_frames.json.

    python tools/gpu_lens_batch.py [--reps 20] [--warmup 3] [--rounds 5] [--out profiles/lens_batch_frames.json]

The method is tools/gpu_wide_aperture.py's: device events around `reps` back-to-back repetitions on one stream (a call
returns before its kernels end: the events end in a synchronise), after `warmup` repetitions of the same shape; the two variants of a
comparison alternate in the same process and the median over `rounds` rounds is reported with the spread of the rounds.
  views    16 and 64 views of 96 x 54 and 16 views of 480 x 270, Float32, max_radius 8 (two launches) and 32 (six): ONE batched device call
           against the loop of n_views single device calls (rtw_wide_aperture_device_*, the parent commit's launches) on the same stream.
           Every view has its own frame -- scene_random_spheres through t_cam1's geometry from a slightly different eye, rendered through the
           pinhole at 1 spp with its real features -- and its own lens: K cycles through max_radius/4, max_radius/2 and max_radius px.
  bracket  one frame under 16 lenses (n_frames == 1: the focus distance runs from 5 to 20) against 16 single calls on that frame.
Before timing, every view of the batch is compared with its single call on the bits (the image and the workspace)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [(16, 96, 54), (64, 96, 54), (16, 480, 270)]
RADII = [8, 32]
CAM = dict(lookat=(0, 0, 0), vup=(0, 1, 0), vfov=20, aspect_ratio=16 / 9, focus_dist=10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens_batch_frames.json"))
    a = ap.parse_args()
    import numpy as np
    import torch                             # (torch's HIP runtime first: INTEGRATION.md section 5)
    import rtw_amd as R
    torch.cuda.init()
    if not torch.cuda.is_available():
        sys.exit("gpu_lens_batch.py measures on a GPU: none found")
    T, dt, eb = np.float32, torch.float32, 4

    def alternate(fns):
        """the variants of a comparison, round-robin, so that a drift of the machine meets all of them"""
        res = {k: [] for k in fns}
        for k, fn in fns.items():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                e1.synchronize()
                res[k].append(e0.elapsed_time(e1) / a.reps)
        return {k: {"ms": statistics.median(v), "min": min(v), "max": max(v)} for k, v in res.items()}

    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "rounds": a.rounds, "precision": "float32",
           "time": "device events around `reps` back-to-back repetitions on the null stream, per repetition (one batched call, or the loop of n_views single calls); "
                   "median (min, max) over the rounds",
           "views": [], "bracket": []}
    scene = R.scene_random_spheres(elem_type=T)
    for n, W, H in CASES:
        cams = [R.default_camera(lookfrom=(13 + 0.05 * v, 2, 3), aperture=0, elem_type=T, **CAM) for v in range(n)]
        images = np.ascontiguousarray(np.swapaxes(R.render_batch(scene, cams, W, 1, seed=1, gamma=False, device=0), 1, 2))
        feats = np.ascontiguousarray(np.swapaxes(R.render_features_batch(scene, cams, W, 1, seed=1, device=0)["raw"], 1, 2))
        d_img, d_feat = torch.from_numpy(images.ravel()).to("cuda:0"), torch.from_numpy(feats.ravel()).to("cuda:0")
        hor = float(np.linalg.norm(np.asarray(cams[0].horizontal, np.float64)))
        for mr in RADII:
            lens = [(mr / 4, mr / 2, mr)[v % 3] * hor / W for v in range(n)]
            one = R.wide_aperture_work_bytes(W, H, T, mr)
            assert R.wide_aperture_batch_work_bytes(W, H, n, T, mr) == n * one
            table = torch.from_numpy(R.lens_table(cams, W, H, lens_radii=lens, max_radius=mr)).to("cuda:0")
            work_b, work_s = (torch.zeros(n * one // eb, dtype=dt, device="cuda:0") for _ in range(2))
            out_b, out_s = (torch.zeros(n * W * H * 3, dtype=dt, device="cuda:0") for _ in range(2))
            frame, ffeat = W * H * 3 * eb, W * H * 8 * eb

            def batch(nf=n, tab=table, img=d_img, ft=d_feat):
                R.wide_aperture_batch_into(out_b.data_ptr(), work_b.data_ptr(), img.data_ptr(), ft.data_ptr(), tab.data_ptr(), W, H, n, n_frames=nf, elem_type=T, max_radius=mr)

            def singles(lens=lens, focus=None, shared=False):
                for v in range(n):
                    R.wide_aperture_into(out_s.data_ptr() + v * frame, work_s.data_ptr() + v * one, d_img.data_ptr() + (0 if shared else v * frame),
                                         d_feat.data_ptr() + (0 if shared else v * ffeat), cams[0 if shared else v], W, H, elem_type=T, max_radius=mr, lens_radius=lens[v],
                                         focus_dist=0.0 if focus is None else focus[v])

            batch(); singles()
            torch.cuda.synchronize()
            assert out_b.cpu().numpy().tobytes() == out_s.cpu().numpy().tobytes() and work_b.cpu().numpy().tobytes() == work_s.cpu().numpy().tobytes(), "the batch differs from the single calls"
            res = alternate({"batch": batch, "singles": singles})
            row = {"n_views": n, "width": W, "height": H, "max_radius": mr, "launches_batch": 2 if mr <= 8 else 6, "launches_singles": n * (2 if mr <= 8 else 6), **res,
                   "singles_over_batch": res["singles"]["ms"] / res["batch"]["ms"]}
            out["views"].append(row)
            print(json.dumps(row), flush=True)
            if n == 16:
                focus = [5.0 + v for v in range(n)]
                k_lens = [(mr / 2) * hor / W] * n
                tab1 = torch.from_numpy(R.lens_table([cams[0]] * n, W, H, lens_radii=k_lens, focus_dists=focus, max_radius=mr)).to("cuda:0")
                b1 = lambda: batch(1, tab1)
                s1 = lambda: singles(k_lens, focus, True)
                b1(); s1()
                torch.cuda.synchronize()
                assert out_b.cpu().numpy().tobytes() == out_s.cpu().numpy().tobytes() and work_b.cpu().numpy().tobytes() == work_s.cpu().numpy().tobytes(), "the bracket differs from the single calls"
                res = alternate({"batch": b1, "singles": s1})
                row = {"n_lenses": n, "width": W, "height": H, "max_radius": mr, **res, "singles_over_batch": res["singles"]["ms"] / res["batch"]["ms"]}
                out["bracket"].append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
