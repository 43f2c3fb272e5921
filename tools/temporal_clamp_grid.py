#!/usr/bin/env python3
"""The temporal clamp's parameter grid on the CPU witness (tests/temporal_clamp_ref.py over oracle renders; no GPU): the table of DESIGN.md 7.21.
usage: python tools/temporal_clamp_grid.py [--out profiles/temporal_clamp_grid.json]

Frame F's scene (tests/features_ref.frame_f) at 64 x 36, Float32, linear, the orbit of tests/test_temporal_ref.py.  Four sequences:
8 frames at 0.75 degrees and 1 spp (DESIGN.md 7.18's row), 16 frames at 3 degrees and 1 spp, 16 at 3 degrees and 4 spp, 16 at 1.5 degrees and
2 spp.  Per sequence the renders and features are made once; then the plain witness and the clamped one for radius 1, 2, 3 x sigma 0.5, 1,
1.5, 2 x guides off / on x len_scale 1, 0.5 accumulate them.  Every figure is the MSE of the last accumulated frame against a 1024-spp oracle
render of the last camera, as a ratio of the MSE of that frame's own image."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

ROWS = [(8, 0.75, 1), (16, 3.0, 1), (16, 3.0, 4), (16, 1.5, 2)]
RADII, SIGMAS, LEN_SCALES = (1, 2, 3), (0.5, 1.0, 1.5, 2.0), (1.0, 0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_clamp_grid.json"))
    a = ap.parse_args()
    import rtw_oracle as O
    import features_ref as FR
    import temporal_clamp_ref as CR
    import temporal_ref as TR
    from conftest import CamObj
    from test_temporal_ref import orbit
    T = np.float32
    W, H = 64, 36
    flat = FR.frame_f(T)[0]
    res = {"tool": "tools/temporal_clamp_grid.py", "frame": "frame F, 64x36, Float32, linear", "figure": "MSE(last accumulated frame) / MSE(last frame's own image), against 1024 spp",
           "rows": {}}
    for n, deg, spp in ROWS:
        t0 = time.time()
        cams = orbit(O, T, n, deg)
        frames = []
        for v, cam in enumerate(cams):
            raw, _ = O.render(flat, cam, W, H, spp, T=T, seed=1 + v, gamma=False)
            feat, poisoned = FR.resolve(FR.items(flat, cam, W, H, spp, 0, 1 + v, T), T)
            assert not poisoned.any()
            frames.append((np.ascontiguousarray(raw), feat, CamObj(cam)))
        truth = O.render(flat, cams[-1], W, H, 1024, T=T, seed=99, gamma=False)[0].astype(np.float64)
        mse = lambda x: float(((x.astype(np.float64) - truth) ** 2).mean())
        mse_raw = mse(frames[-1][0])

        def run(step):
            st = prev = out = None
            for raw, feat, cam in frames:
                out, st = step(raw, feat, cam, st, prev)
                prev = cam
            return round(mse(out) / mse_raw, 4)

        row = {"plain": run(lambda raw, feat, cam, st, prev: TR.step(raw, feat, cam, T, st, prev, gamma=0)), "clamped": {}}
        for r in RADII:
            for g in (False, True):
                for ls in LEN_SCALES:
                    for sg in SIGMAS:
                        ck = dict(radius=r, guides=g, sigma=sg, len_scale=ls)
                        row["clamped"][f"r={r} guides={int(g)} len_scale={ls} sigma={sg}"] = run(
                            lambda raw, feat, cam, st, prev: CR.step_clamped(raw, feat, cam, T, st, prev, gamma=0, clamp=ck)[:2])
        res["rows"][f"{n} frames, {deg} deg/frame, {spp} spp"] = row
        print(f"{n} frames {deg} deg {spp} spp: plain {row['plain']}  defaults {row['clamped']['r=1 guides=0 len_scale=1.0 sigma=1.0']}  "
              f"best {min(row['clamped'].items(), key=lambda kv: kv[1])}  ({time.time() - t0:.0f} s)", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
