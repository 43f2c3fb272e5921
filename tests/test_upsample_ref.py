"""The witness of the feature-guided upsampler (tests/upsample_ref.py), CPU only: its two forms agree on the bits, the integer coordinates
have the properties include/rtw_hip.h states, the committed hand-made pairs reach every branch the GPU comparison is meant to cover, and
a step in albedo and normal is not crossed."""
import numpy as np
import pytest

import denoise_ref as DR
import upsample_ref as UR


@pytest.mark.parametrize("levels", [0, 2])
@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("lo,hi", [((5, 3), (11, 7)), ((7, 5), (7, 5))])
def test_vectorised_equals_scalar_on_the_bits(lo, hi, T, levels):
    (w, h), (W, H) = lo, hi
    pair = UR.handmade_pair(h, w, H, W, T, UR.SEEDS[T])
    seen_nan = seen_finite = False
    for m, demodulate, gamma in ((1, True, 1), (0, False, 0), (7, True, 0)):
        kw = dict(levels=levels, m=m, demodulate=demodulate, gamma=gamma)
        a, b = UR.upsample(*pair, T, **kw), UR.upsample_scalar(*pair, T, **kw)
        assert a.dtype == np.dtype(T) and a.shape == (H, W, 3)
        assert UR.same_bits(a, b), kw
        seen_nan, seen_finite = seen_nan or bool(np.isnan(a).any()), seen_finite or bool(np.isfinite(a).any())
    assert seen_finite and (seen_nan or H * W < 12)


def test_sigmas_reach_the_witness():
    T = np.float32
    pair = UR.handmade_pair(10, 18, 23, 37, T, UR.SEEDS[T])
    base = UR.upsample(*pair, T)
    for kw in (dict(sigma_albedo=2.0), dict(sigma_depth=3.0), dict(sigma_color=4.0), dict(levels=0), dict(m=3)):
        assert not UR.same_bits(UR.upsample(*pair, T, **kw), base), kw


def test_coordinates():
    """for every pair 1 <= w <= W <= 64: x0 in [-2, w-1], r_x in [0, 2W), kx >= 0, and a tap inside the small frame with a positive
    weight; equal sizes give fx = 0 and x0 = j"""
    for T in (np.float32, np.float64):
        for W in range(1, 65):
            for w in range(1, W + 1):
                x0, r, fx = UR.coords(w, W, T)
                assert x0.min() >= -2 and x0.max() <= w - 1, (w, W)
                assert (fx >= 0).all() and (fx < 1).all()
                best = np.zeros(W, T)
                for b in range(-1, 3):
                    kx = UR.tent(b, fx, T)
                    assert (kx >= 0).all(), (w, W, b)
                    inside = (x0 + b >= 0) & (x0 + b < w)
                    best = np.maximum(best, np.where(inside, kx, T(0)))
                assert (best > 0).all(), (w, W)
            x0, r, fx = UR.coords(W, W, T)
            assert np.array_equal(x0, np.arange(W)) and (fx == 0).all() and (r == 0).all()
    # the 2x case by hand: num_x = 10j - 15, so x0 + fx = (2j - 3) / 4
    x0, r, fx = UR.coords(5, 10, np.float64)
    assert x0.tolist() == [-1, -1, 0, 0, 1, 1, 2, 2, 3, 3] and fx.tolist() == [0.25, 0.75] * 5


BIG_PAIRS = [(lo, hi) for lo, hi in UR.PAIRS if hi[0] * hi[1] >= 37 * 23]


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("lo,hi", BIG_PAIRS)
def test_the_committed_seeds_reach_every_branch(lo, hi, T):
    """without this the GPU comparison would show nothing about the fallback, the two kinds of NaN pixel and a subnormal sum_w"""
    (w, h), (W, H) = lo, hi
    pair = UR.handmade_pair(h, w, H, W, T, UR.SEEDS[T])
    c = UR.census(*pair, T, levels=0, m=7)
    assert all(v >= 1 for v in c.values()), c
    small = DR.census(pair[0], pair[1])
    assert small["cov0"] and small["cov_frac"] and small["cov1"] and small["tiny_albedo"] and small["z_le_0"] and small["non_finite"], small
    # the normal weight alone makes sum_w subnormal: with m = 1 the same pixels have a normal one
    assert UR.census(*pair, T, levels=0, m=1)["subnormal_sum_w"] == 0


def test_the_big_pairs_are_the_ones_expected():
    assert BIG_PAIRS == [((18, 10), (37, 23)), ((35, 20), (70, 41)), ((70, 41), (70, 41)), ((9, 40), (10, 300))]
    assert len(UR.PAIRS) == 8


@pytest.mark.parametrize("m", [0, 1, 7])
@pytest.mark.parametrize("levels", [0, 2])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_step_is_not_crossed(T, levels, m):
    """A full-size step frame (denoise_ref.step_frame: orthogonal normals on the two sides) with its box-averaged half-size counterpart:
    every cross-edge weight is exactly 0, so each output channel on one side is a weighted mean of that side's small-frame values e*a.
    It lies within their range, widened by a relative 64 eps(T): 16 products, 16 sums and a quotient, each rounded once (and the product
    with the albedo)."""
    noisy, _, feat_hi = DR.step_frame(T, 5)
    H, W = feat_hi.shape[:2]
    image_lo, feat_lo = UR.box_half(noisy), UR.box_half(feat_hi)
    assert image_lo.dtype == np.dtype(T) and feat_lo.shape == (H // 2, W // 2, 8)
    d = {}
    out = UR.upsample(image_lo, feat_lo, feat_hi, T, levels=levels, m=m, gamma=0, details=d)
    assert np.isfinite(out).all() and d["guided"].all()
    ea = d["e"] * d["a"]                                   # what the taps read, modulated: [h, w, 3]
    eps = np.finfo(T).eps
    for side_hi, side_lo in ((np.s_[:, :W // 2], np.s_[:, :W // 4]), (np.s_[:, W // 2:], np.s_[:, W // 4:])):
        for k in range(3):
            lo, hi = float(ea[side_lo][..., k].min()), float(ea[side_lo][..., k].max())
            got = out[side_hi][..., k].astype(np.float64)
            assert (got >= lo * (1 - 64 * eps)).all() and (got <= hi * (1 + 64 * eps)).all(), (k, lo, hi, got.min(), got.max())
    # and the two sides do differ: the ranges above do not overlap in the first channel
    assert ea[:, :W // 4, 0].min() > ea[:, W // 4:, 0].max()
