"""The witness of the motion-blur stage (tests/motion_blur_ref.py; include/rtw_hip.h rtw_velocity_blur_*) on the CPU: it agrees with itself
(vectorised against scalar, on the bits), its hand-made cases reach every regime the GPU test relies on, it is the identity where nothing
moves, it spreads an impulse over the expected line, and it brings a sharp frame of a moving scene closer to the time-averaged truth.  No GPU."""
import functools
import time

import numpy as np
import pytest

import features_ref as FR
import motion_blur_ref as BR
import motion_ref as MR
from conftest import CamObj
from test_motion_ref import animated_scenes
from test_temporal_ref import orbit

PRECISIONS = [np.float32, np.float64]
REGIMES = ["pass_tiles", "filter_tiles", "clamped", "from_neighbour", "tile_ties", "taps_outside", "taps_invalid", "sphere_over_sky", "sky_over_sphere", "both_sky",
           "soft_depth", "rint_ties", "not_front", "nan_slot", "invalid"]


@functools.lru_cache(maxsize=None)
def _cases(size, T):
    W, H = size
    return BR.handmade_blur_cases(H, W, T, BR.SEEDS[T])


def _args(c, T):
    return (c["image"], c["features"], c["motion"], c["cam"], c["cam_prev"], T)


# ---- 1. the witness agrees with itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", BR.SIZES)
@pytest.mark.parametrize("T", PRECISIONS)
def test_vectorised_equals_scalar_on_the_bits(T, size):
    """the image, the blur plane, the tile plane and the neighbour plane of every hand-made case"""
    for k, c in enumerate(_cases(size, T)):
        assert BR.same_blur(BR.blur(*_args(c, T), **c["params"]), BR.blur_scalar(*_args(c, T), **c["params"])), (size, k)


@pytest.mark.parametrize("T", PRECISIONS)
def test_census_of_the_hand_made_cases(T):
    """over the cases of all frame sizes together, every regime at least once (a condition: the seeds are picked so that it holds)"""
    total = dict.fromkeys(REGIMES, 0)
    for size in BR.SIZES:
        for k, c in enumerate(_cases(size, T)):
            cen = BR.census(c, T)
            print(np.dtype(T).name, size, "case", k, cen)
            for r in REGIMES:
                total[r] += cen[r]
    print(np.dtype(T).name, "total", total)
    assert all(total[r] >= 1 for r in REGIMES), total
    # half-extents from 0 to the clamp at 16 px
    ls = np.concatenate([BR.blur_plane(*_args(c, T), shutter=c["params"]["shutter"])[..., 3].ravel() for size in BR.SIZES for c in _cases(size, T)])
    assert ls.min() == 0 and ls.max() >= 15.99 and ((ls > 0.5) & (ls < 4)).any() and ((ls > 4) & (ls < 15)).any()


# ---- 2. where nothing moves --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(5, 3), (37, 23), (70, 40)])
@pytest.mark.parametrize("T", PRECISIONS)
def test_zero_motion_and_one_camera_is_the_identity_on_the_bits(T, size):
    """a zero motion plane and cam_prev == cam: every tile passes through -- the input on the bits, its sqrt with gamma 1; NaN where not valid"""
    c = _cases(size, T)[0]
    zero = np.zeros_like(c["motion"])
    for taps in (3, 15, 31):
        out, work = BR.blur(c["image"], c["features"], zero, c["cam"], c["cam"], T, taps=taps)
        valid = ~np.isnan(work["plane"][..., 2])
        assert (work["nb"][..., 2] < 0.5).all() and valid.any()
        assert BR.same_bits(out[valid], c["image"][valid]) and np.isnan(out[~valid]).all()
        out, _ = BR.blur(c["image"], c["features"], zero, c["cam"], c["cam"], T, taps=taps, gamma=1)
        with np.errstate(invalid="ignore"):
            assert BR.same_bits(out[valid], np.sqrt(c["image"][valid]))


@pytest.mark.parametrize("T", PRECISIONS)
def test_a_uniform_velocity_blurs_an_impulse_into_a_line(rtw, T):
    """a flat wall at depth 1 that moved 8 px to the right, one white pixel on black: shutter 1 gives a half-extent of 4 px, so the
    impulse spreads over the row's columns j0 - 4 .. j0 + 4 at most and over j0 - 3 .. j0 + 3 at least (15 taps: one tap per 0.5 px), stays in
    its row, and keeps its energy within the taps' weights: every blurred value is in [0, 1]"""
    import temporal_ref as TR
    W, H, j0, i0 = 48, 32, 24, 16
    cam = TR.make_camera(rtw, T, (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), W, H)
    image = np.zeros((H, W, 3), T)
    image[i0, j0] = 1
    feat = np.zeros((H, W, 8), T)
    feat[..., 0:3], feat[..., 5], feat[..., 7] = 0.5, 1.0, 1.0
    rays = MR.centre_rays(cam, W, H, T).astype(np.float64)
    feat[..., 6] = (1.0 / -rays[..., 5]).astype(T)                      # the plane z = -1 seen from the origin: distance along the ray
    motion = np.zeros((H, W, 4), T)
    motion[..., 0] = (8.0 * np.asarray(cam.horizontal, np.float64)[0] / W)      # 8 px at distance 1 along w (focus_dist is 1)
    d = {}
    out, work = BR.blur(image, feat, motion, cam, cam, T, details=d)
    hx = work["plane"][..., 0]
    assert np.abs(hx - 4).max() < 1e-3 and np.abs(work["plane"][..., 1]).max() < 1e-3, (hx.min(), hx.max())
    lit = np.argwhere(out[..., 0] > 0)
    assert (lit[:, 0] == i0).all()
    cols = sorted(lit[:, 1])
    print(np.dtype(T).name, "lit columns", cols, "values", out[i0, cols[0]:cols[-1] + 1, 0])
    assert cols[0] >= j0 - 4 and cols[-1] <= j0 + 4 and cols[0] <= j0 - 3 and cols[-1] >= j0 + 3 and cols == list(range(cols[0], cols[-1] + 1))
    assert (out >= 0).all() and (out <= 1).all() and out[i0, j0, 0] < 1
    assert BR.same_blur((out, work), BR.blur_scalar(image, feat, motion, cam, cam, T))


# ---- 3. it helps -----------------------------------------------------------------------------------------------------------------------------------
def test_it_brings_a_sharp_frame_closer_to_the_time_averaged_truth(oracle):
    """Frame F's scene with its spheres moving at twice test_motion_ref's speed, frame 1 against frame 0, a fixed pinhole camera, 128 x 72,
    shutter 1, 15 taps, depth extent 0.5, the witness in binary32.  Truth: the mean of 8 oracle renders at the sub-frame times
    tau = (k + 0.5)/8 - 0.5 (centres c1 + tau (c1 - c0)), 64 spp each.  Strictly: the blurred frame's MSE to the truth is below the sharp
    frame's, over the whole frame and over the pixels whose own motion exceeds half a pixel, for a 1024-spp input and for a 4-spp input
    (features: the feature witness at min(spp, 16) samples); and the noise floor (the MSE between two independent truths) is below the
    gap asserted on the 1024-spp rows.  The ratios are printed."""
    T = np.float32
    W, H, SUB, SPP = 128, 72, 8, 64
    t0 = time.time()
    scenes, _ = animated_scenes(T, 2, speed=2.0)
    cam = orbit(oracle, T, 1)[0]

    def truth(seed0):
        acc = np.zeros((H, W, 3), np.float64)
        for k in range(SUB):
            tau = (k + 0.5) / SUB - 0.5
            s = {n: (np.asarray(a).copy() if isinstance(a, np.ndarray) else a) for n, a in scenes[1].items()}
            for n in ("cx", "cy", "cz"):
                c0, c1 = np.asarray(scenes[0][n], np.float64), np.asarray(scenes[1][n], np.float64)
                s[n] = (c1 + tau * (c1 - c0)).astype(T)
            acc += oracle.render(s, cam, W, H, SPP, T=T, seed=seed0 + k, gamma=False)[0].astype(np.float64)
        return acc / SUB
    truth_a, truth_b = truth(1000), truth(2000)
    floor = float(((truth_a - truth_b) ** 2).mean())
    motion = MR.motion_pass(scenes[1], cam, W, H, T, MR.motion_table(scenes[0], scenes[1], T))
    camo = CamObj(cam)
    rows = {}
    for spp in (1024, 4):
        sharp, _ = oracle.render(scenes[1], cam, W, H, spp, T=T, seed=7, gamma=False)
        fspp = min(spp, 16)                                 # (a 16-sample feature pass: the feature witness at 1024 spp takes minutes)
        feat, poisoned = FR.resolve(FR.items(scenes[1], cam, W, H, fspp, 0, 7, T), T)
        assert not poisoned.any()
        sharp = np.ascontiguousarray(sharp)
        blurred, work = BR.blur(sharp, feat, motion, camo, camo, T, taps=15, shutter=1.0, depth_extent=0.5)
        own = work["plane"][..., 3] > 0.25                      # shutter 1: l = |u| / 2 (a clamped l is 16)
        assert np.isfinite(blurred).all()
        mse = lambda a, m: float(((a.astype(np.float64) - truth_a) ** 2)[m].mean())
        everything = np.ones((H, W), bool)
        rows[spp] = [(mse(sharp, m), mse(blurred, m)) for m in (everything, own)]
        print(f"{spp} spp: largest half-extent {float(work['plane'][..., 3].max()):.2f} px, {int(own.sum())} pixels move by more than half a pixel, "
              f"{int((work['nb'][..., 2] >= 0.5).sum())} of {work['nb'].shape[0] * work['nb'].shape[1]} tiles filter")
        for name, (a, b) in zip(("whole frame", "own motion > 0.5 px"), rows[spp]):
            print(f"  {name:20s} MSE sharp {a:.6f}  blurred {b:.6f}  ratio {b / a:.3f}")
    print(f"noise floor (two independent truths): {floor:.6f}  ({time.time() - t0:.1f} s)")
    for spp in (1024, 4):
        for a, b in rows[spp]:
            assert b < a
    assert all(floor < a - b for a, b in rows[1024])
