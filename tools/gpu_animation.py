#!/usr/bin/env python3
"""Temporal reuse over moving spheres on one MI355X (include/rtw_hip.h rtw_first_hit_motion_*, rtw_animated_step_*, rtw_render_animation_*): the measurements of
DESIGN.md 7.23, written to profiles/animation_frames.json.

    python tools/gpu_animation.py [--reps 200] [--warmup 20] [--out profiles/animation_frames.json]

Everything is timed by device events around `reps` back-to-back launches on one stream (a launch returns before its kernel ends: the events
end in a synchronise), after `warmup` launches of the same shape; the variants of a comparison alternate in the same process and the median
over 5 rounds is reported with the spread of the rounds.
  pass    the motion pass on the 485-sphere scene at 1920 x 1080 and 480 x 270, Float32 and Float64, next to its yardstick: the 1-chunk feature
          pass of the same frame (spp = 1).  No ratio is asked for; it is recorded.
  step    the motion step against the plain step, and the clamped motion step (r = 1) against the clamped step, at 1920 x 1080: the motion
          step adds one 16- / 32-byte load per pixel, bytes_per_pixel says what each moves.
  chain   8 frames of an animation (a new scene per frame) at 480 x 270, 1 spp, Float32, wall clock around the blocking call:
          rtw.render_animation (ONE call of rtw_render_animation_*; from HittableLists and from scenes flattened beforehand) against the chain of
          the single host-array calls it replaces, against itself over 8 IDENTICAL scenes (no upload after the first call: the difference,
          over 8, is what one per-frame upload costs inside the call) and against rtw.render_sequence of 8 views of ONE scene (one batched
          render and feature pass instead of 8 + 8 launches, no motion pass)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "animation_frames.json"))
    a = ap.parse_args()
    import numpy as np
    import torch                             # (torch's HIP runtime first: INTEGRATION.md section 5)
    import rtw_amd as R
    torch.cuda.init()
    if not torch.cuda.is_available():
        sys.exit("gpu_animation.py measures on a GPU: none found")

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

    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "rounds": a.rounds,
           "time": "device events around `reps` back-to-back launches on the null stream, per launch; median (min, max) over the rounds; chain: wall clock, median of 7",
           "pass": [], "step": [], "chain": {}}
    for T, dt in ((np.float32, torch.float32), (np.float64, torch.float64)):
        eb = np.dtype(T).itemsize
        R.reseed()
        scene = R.scene_random_spheres(elem_type=T)
        cam = R.default_camera(lookfrom=(13, 2, 3), lookat=(0, 0, 0), vfov=20, aperture=0, focus_dist=10, elem_type=T)
        cam2 = R.default_camera(lookfrom=(13.04, 2, 2.83), lookat=(0, 0, 0), vfov=20, aperture=0, focus_dist=10, elem_type=T)
        ren = R.DeviceRenderer(scene, cam, device=0)
        n = ren.n_spheres
        table = torch.from_numpy(np.random.default_rng(1).uniform(-0.1, 0.1, (n, 4)).astype(T)).to("cuda:0")
        for W in (1920, 480):
            H = R.image_height(W)
            motion = torch.zeros(W * H * 4, dtype=dt, device="cuda:0")
            feat = torch.zeros(W * H * 8, dtype=dt, device="cuda:0")
            res = alternate({"motion_pass": lambda: R.first_hit_motion_into(ren, motion.data_ptr(), W, H, d_table_ptr=table.data_ptr()),
                             "feature_pass_1_chunk": lambda: R.features_into(ren, feat.data_ptr(), W, 1)})
            out["pass"].append({"precision": np.dtype(T).name, "width": W, "height": H, "spheres": n, **res,
                                "ratio_to_feature_pass": res["motion_pass"]["ms"] / res["feature_pass_1_chunk"]["ms"]})
            print(out["pass"][-1], flush=True)
        W = 1920
        H = R.image_height(W)
        img = torch.zeros(W * H * 3, dtype=dt, device="cuda:0")
        ren.render_into(img.data_ptr(), W, 1, gamma=False)
        feat = torch.zeros(W * H * 8, dtype=dt, device="cuda:0")
        R.features_into(ren, feat.data_ptr(), W, 1)
        motion = torch.zeros(W * H * 4, dtype=dt, device="cuda:0")
        R.first_hit_motion_into(ren, motion.data_ptr(), W, H, d_table_ptr=table.data_ptr())
        ns = R.temporal_state_bytes(W, H, T) // eb
        s0, s1, o = (torch.zeros(k, dtype=dt, device="cuda:0") for k in (ns, ns, W * H * 3))
        torch.cuda.synchronize()
        R.temporal_step_into(o.data_ptr(), s0.data_ptr(), img.data_ptr(), feat.data_ptr(), cam2, W, H, elem_type=T)
        kw = dict(d_state_prev_ptr=s0.data_ptr(), cam_prev=cam2, elem_type=T)
        args = (o.data_ptr(), s1.data_ptr(), img.data_ptr(), feat.data_ptr(), cam, W, H)
        res = alternate({"plain": lambda: R.temporal_step_into(*args, **kw),
                         "motion": lambda: R.temporal_step_animated_into(*args, d_motion_ptr=motion.data_ptr(), **kw),
                         "clamped_r1": lambda: R.temporal_step_clamped_into(*args, clamp=True, **kw),
                         "clamped_r1_motion": lambda: R.temporal_step_animated_into(*args, d_motion_ptr=motion.data_ptr(), clamp=True, **kw)})
        # per pixel: image 3 + features 8 + out 3 + next state 9 elements, four taps of 9 elements (mostly from L2), the slot 4
        out["step"].append({"precision": np.dtype(T).name, "width": W, "height": H, **res, "bytes_per_pixel_without_taps": (3 + 8 + 3 + 9) * eb,
                            "bytes_per_pixel_of_the_slot": 4 * eb, "motion_over_plain": res["motion"]["ms"] / res["plain"]["ms"],
                            "clamped_motion_over_clamped": res["clamped_r1_motion"]["ms"] / res["clamped_r1"]["ms"]})
        print(out["step"][-1], flush=True)
        del ren
    # the one call against the chain of single calls, against itself without uploads and against the sequence of a static scene
    T = np.float32
    R.reseed()
    base = R.scene_random_spheres(elem_type=T)
    cams = [R.default_camera(lookfrom=(13, 2, 3), lookat=(0, 0, 0), vfov=20, aperture=0, focus_dist=10, elem_type=T)] * 8
    scenes = []
    for v in range(8):
        sc = R.HittableList([R.Sphere(np.asarray(s.center) + (np.array([0.02 * v, 0, 0], dtype=T) if k % 7 == 3 else 0), s.radius, s.mat) for k, s in enumerate(base)])
        scenes.append(sc)
    flats = [R.flatten_scene(sc, T) for sc in scenes]
    W = 480
    H = R.image_height(W)

    def chain():
        frames, state = [], None
        for v, (scene, cam) in enumerate(zip(scenes, cams)):
            img = R.render(scene, cam, W, 1, gamma=False, device=0)
            feat = R.render_features(scene, cam, W, 1, device=0)["raw"]
            mv = R.first_hit_motion(flats[v], cam, W, H, table=R.motion_table(flats[v - 1], flats[v], T), device=0) if v else None
            o, state = R.temporal_step_animated(img, feat, cam, mv, state, None, cams[v - 1] if v else None, device=0)
            frames.append(o)
        return np.stack(frames)

    assert np.array_equal(chain(), R.render_animation(flats, cams, W, 1, device=0))
    for name, fn in (("render_animation_one_call", lambda: R.render_animation(scenes, cams, W, 1, device=0)),
                     ("render_animation_one_call_flat_scenes", lambda: R.render_animation(flats, cams, W, 1, device=0)),
                     ("render_animation_one_call_flat_identical_scenes", lambda: R.render_animation(flats[:1] * 8, cams, W, 1, device=0)),
                     ("chain_of_single_calls", chain),
                     ("render_sequence_static", lambda: R.render_sequence(base, cams, W, 1, device=0))):
        fn()
        fn()
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        out["chain"][name] = {"ms": statistics.median(ts), "min": min(ts), "max": max(ts), "frames": 8, "width": W, "spp": 1, "spheres": len(base)}
    c = out["chain"]
    c["upload_per_frame_ms"] = (c["render_animation_one_call_flat_scenes"]["ms"] - c["render_animation_one_call_flat_identical_scenes"]["ms"]) / 8
    print(out["chain"], flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
