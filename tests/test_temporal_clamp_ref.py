"""The temporal clamp's witness (tests/temporal_clamp_ref.py) against itself, against the plain witnesses and against the CPU oracle, no GPU:
the vectorised restatement equals the scalar one on the bits; the committed inputs reach every regime of the definition (counted, so an input
that stops reaching one fails); a step that moves no pixel is the plain step on the bits; a constant frame pulls every accepted history onto
itself; every parameter matters; and along a real 4-spp camera path the clamped accumulation is closer to a 1024-spp render than the plain one."""
import functools
import time

import numpy as np
import pytest

import features_ref as FR
import temporal_clamp_ref as CR
import temporal_noise_ref as NR
import temporal_ref as TR
from conftest import CamObj
from test_temporal_ref import orbit

SIZES = [(3, 2), (1, 1), (70, 40), (64, 36)]


@functools.lru_cache(maxsize=None)
def _sequence(size, T):
    W, H = size
    return NR.handmade_sequence(H, W, T, CR.SEEDS[T], 3)


# ---- 1. the two restatements agree on the bits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("guides", [False, True])
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_vectorised_equals_scalar_on_the_bits(T, size, radius, guides, moments):
    cams, frames, state0, moment0, cam0 = _sequence(size, T)
    ck = dict(radius=radius, guides=guides, sigma=1.0, len_scale=0.5)
    mo = moment0 if moments else None
    a = CR.step_clamped(*frames[0], cams[0], T, state0, cam0, mo, clamp=ck)
    b = CR.step_clamped_scalar(*frames[0], cams[0], T, state0, cam0, mo, clamp=ck)
    assert a[0].dtype == b[0].dtype == np.dtype(T) and (a[2] is not None) == moments
    assert CR.same_step(a, b)
    # with moments the image and the state are those without, on the bits
    if moments:
        c = CR.step_clamped(*frames[0], cams[0], T, state0, cam0, None, clamp=ck)
        assert TR.same_bits(a[0], c[0]) and TR.same_state(a[1], c[1]) and c[2] is None
    # the first frame is the plain step's, and the second step of the chain agrees too (the state a step left, not a hand-made one)
    f = CR.step_clamped(*frames[0], cams[0], T, moments=moments, clamp=ck)
    p = NR.step_moments(*frames[0], cams[0], T)
    assert TR.same_bits(f[0], p[0]) and TR.same_state(f[1], p[1]) and (not moments or TR.same_bits(f[2], p[2]))
    a2 = CR.step_clamped(*frames[1], cams[1], T, a[1], cams[0], a[2], clamp=ck)
    b2 = CR.step_clamped_scalar(*frames[1], cams[1], T, a[1], cams[0], a[2], clamp=ck)
    assert CR.same_step(a2, b2)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_forms_agree_on_the_planted_step_and_under_every_mode(T):
    cam, cp, img, feat, st, mo = CR.planted_sequence(T)
    for ck in (dict(radius=1), dict(radius=2, guides=True, sigma=0.5, len_scale=0.0), dict(radius=3, guides=True, sigma=0.0), dict(radius=3, sigma=2.0, len_scale=0.25)):
        for kw in (dict(), dict(demodulate=False, gamma=0), dict(m=0, sigma_depth=0.5), dict(m=7, history_max=3.5, min_weight=0.6)):
            a = CR.step_clamped(img, feat, cam, T, st, cp, mo, clamp=ck, **kw)
            b = CR.step_clamped_scalar(img, feat, cam, T, st, cp, mo, clamp=ck, **kw)
            assert CR.same_step(a, b), (ck, kw)


# ---- 2. the committed inputs reach every regime -------------------------------------------------------------------------------------------
REGIMES = ("accepted", "reset", "clamped_lo", "clamped_hi", "untouched", "nan_bounds", "sd_zero", "cut_top", "cut_bottom", "cut_left", "cut_right",
           "frame_smaller_than_window", "invalid_neighbour", "invalid_centre", "sky_covered_pair", "len_shortened", "first_frame")


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_census_reaches_every_regime(T):
    """a weakened generator fails here.  The inputs are those the GPU comparison sweeps: step 0 of the hand-made sequences, the planted step and
    a first frame; every regime is reached by at least one of them, and the ones each input is there for are asserted input by input."""
    ck = dict(sigma=1.0, len_scale=0.5)
    total = dict.fromkeys(REGIMES, 0)

    def add(c):
        for k, v in c.items():
            total[k] += v
        return c

    for size in SIZES:
        cams, frames, state0, moment0, cam0 = _sequence(size, T)
        for radius in (1, 2, 3):
            for guides in (False, True):
                c = add(CR.census(*frames[0], cams[0], T, state0, cam0, moment0, clamp=dict(ck, radius=radius, guides=guides)))
                if size == (3, 2):
                    assert c["frame_smaller_than_window"] >= 1 and c["clamped_lo"] >= 1 and c["len_shortened"] >= 1, c
                if size in ((70, 40), (64, 36)):
                    for key in ("accepted", "reset", "clamped_lo", "clamped_hi", "untouched", "cut_top", "cut_bottom", "cut_left", "invalid_neighbour", "invalid_centre",
                                "sky_covered_pair", "len_shortened"):
                        assert c[key] >= 1, (key, c)
        add(CR.census(*frames[0], cams[0], T, None, None))
    cam, cp, img, feat, st, mo = CR.planted_sequence(T)
    for radius in (1, 2, 3):
        for guides in (False, True):
            c = add(CR.census(img, feat, cam, T, st, cp, mo, clamp=dict(ck, radius=radius, guides=guides)))
            for key in ("clamped_lo", "clamped_hi", "untouched", "sd_zero", "cut_top", "cut_bottom", "cut_left", "cut_right", "invalid_neighbour", "invalid_centre",
                        "sky_covered_pair", "len_shortened", "reset"):
                assert c[key] >= 1, (key, c)
            assert c["nan_bounds"] == (1 if guides else 0), c         # S0 = 0 needs weights: the unweighted window counts its centre
    for key in REGIMES:
        assert total[key] >= 1, (key, total)
    # len_scale = 1 shortens nothing
    c = CR.census(img, feat, cam, T, st, cp, mo, clamp=dict(radius=1))
    assert c["len_shortened"] == 0 and c["clamped_hi"] >= 1


# ---- 3. properties of the definition --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guides", [False, True])
@pytest.mark.parametrize("size", [(12, 9), (70, 40)])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_step_that_moves_no_pixel_is_the_plain_step_on_the_bits(T, size, guides):
    W, H = size
    cam, cp, img, feat, st, mo = CR.no_movement_sequence(H, W, T)
    for radius in (1, 3):
        ck = dict(radius=radius, guides=guides, sigma=1.0, len_scale=0.5)
        d = {}
        a = CR.step_clamped(img, feat, cam, T, st, cp, mo, clamp=ck, details=d)
        assert d["accept"].all() and not d["moved"].any() and (d["sd"] == 0).all()      # (the premise, on the witness)
        p = NR.step_moments(img, feat, cam, T, st, mo, cp)
        assert CR.same_step(a, p)
        q = TR.step(img, feat, cam, T, st, cp)
        b = CR.step_clamped(img, feat, cam, T, st, cp, clamp=ck)
        assert b[2] is None and TR.same_bits(b[0], q[0]) and TR.same_state(b[1], q[1])
    assert (a[1]["L"] > 1).all()


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_constant_frame_pulls_every_accepted_history_onto_itself(T):
    cam, cp, img, feat, st = CR.constant_sequence(9, 12, T)
    for demodulate in (True, False):
        d = {}
        out, nxt, _ = CR.step_clamped(img, feat, cam, T, st, cp, demodulate=demodulate, gamma=0, details=d)
        assert d["accept"].all() and (d["eh"] == 2).all()
        assert (d["hc"] == T(0.5)).all() and d["moved"].all()
        assert (out == T(0.5)).all() and (nxt["E"][..., 0:3] == T(0.5)).all()
    plain, _ = TR.step(img, feat, cam, T, st, cp, gamma=0)
    assert (plain > T(0.5)).all()


def test_the_parameters_matter():
    T = np.float32
    cams, frames, state0, moment0, cam0 = _sequence((70, 40), T)
    base_k = dict(radius=1, guides=False, sigma=1.0, len_scale=1.0)
    base = CR.step_clamped(*frames[0], cams[0], T, state0, cam0, moment0, clamp=base_k)
    plain = NR.step_moments(*frames[0], cams[0], T, state0, moment0, cam0)
    assert not CR.same_step(base, plain)
    for kw in (dict(radius=2), dict(radius=3), dict(guides=True), dict(sigma=0.5), dict(sigma=2.0), dict(len_scale=0.5), dict(len_scale=0.0)):
        got = CR.step_clamped(*frames[0], cams[0], T, state0, cam0, moment0, clamp=dict(base_k, **kw))
        assert not CR.same_step(got, base), kw
    # len_scale touches len and alpha, and through alpha the colour and the moment -- but never the guides
    got = CR.step_clamped(*frames[0], cams[0], T, state0, cam0, moment0, clamp=dict(base_k, len_scale=0.5))
    assert TR.same_bits(got[1]["G"], base[1]["G"]) and not TR.same_bits(got[1]["L"], base[1]["L"])
    # the window's weights are the step's m and sigma_depth
    g = dict(base_k, guides=True)
    a, b = (CR.step_clamped(*frames[0], cams[0], T, state0, cam0, moment0, clamp=g, **kw)[0] for kw in (dict(), dict(m=3)))
    assert not TR.same_bits(a, b)


# ---- 4. it helps ------------------------------------------------------------------------------------------------------------------------------
def test_it_helps_along_an_orbit(oracle):
    """16 pinhole cameras of test_temporal_ref.orbit at 3 degrees per frame over frame F's scene at 64 x 36, 4 spp each, Float32, linear,
    defaults everywhere: frame 16 accumulated by the clamped witness against the plain witness's, both against a 1024-spp oracle render of
    camera 16.  The condition is MSE(clamped) < MSE(plain), strictly, both finite; the ratios to the frame's own image are printed
    (DESIGN.md 7.21), not fixed."""
    T = np.float32
    flat = FR.frame_f(T)[0]
    W, H = 64, 36
    cams = orbit(oracle, T, 16, 3.0)
    t0 = time.time()
    sp = sc = prev = out_p = out_c = raw = None
    for v, cam in enumerate(cams):
        raw, _ = oracle.render(flat, cam, W, H, 4, T=T, seed=1 + v, gamma=False)
        feat, poisoned = FR.resolve(FR.items(flat, cam, W, H, 4, 0, 1 + v, T), T)
        assert not poisoned.any()
        raw = np.ascontiguousarray(raw)
        out_p, sp = TR.step(raw, feat, CamObj(cam), T, sp, prev, gamma=0)
        out_c, sc, _ = CR.step_clamped(raw, feat, CamObj(cam), T, sc, prev, gamma=0)
        prev = CamObj(cam)
    truth, _ = oracle.render(flat, cams[-1], W, H, 1024, T=T, seed=99, gamma=False)
    truth = truth.astype(np.float64)
    mse = lambda x: float(((x.astype(np.float64) - truth) ** 2).mean())
    mse_raw, mse_p, mse_c = mse(raw), mse(out_p), mse(out_c)
    print(f"MSE frame 16 at 4 spp {mse_raw:.6f}  plain {mse_p:.6f} (ratio {mse_p / mse_raw:.3f})  clamped {mse_c:.6f} (ratio {mse_c / mse_raw:.3f})  ({time.time() - t0:.1f} s)")
    assert np.isfinite(out_p).all() and np.isfinite(out_c).all() and np.isfinite(mse_p) and np.isfinite(mse_c)
    assert mse_c < mse_p
