"""The temporal moments' witness (tests/temporal_noise_ref.py) against itself, against temporal_ref, against exact rational arithmetic and
against the CPU oracle, no GPU: the vectorised restatements equal the scalar ones on the bits; the step with moments leaves temporal_ref's
image and state; the committed seeds reach every regime of the two definitions; on constant frames the moments are the population variance
within a derived rounding bound; and along a real 1-spp camera path the guided filter behind the new map is closer to a 1024-spp render than
the last frame itself (the three ratios are DESIGN.md 7.19's record)."""
import functools
import time
from fractions import Fraction

import numpy as np
import pytest

import accum_denoise_ref as AR
import denoise_ref as DR
import features_ref as FR
import temporal_noise_ref as NR
import temporal_ref as TR
from conftest import CamObj


@functools.lru_cache(maxsize=None)
def _sequence(size, T):
    W, H = size
    return NR.handmade_sequence(H, W, T, NR.SEEDS[T], 3)


# ---- 1. the two restatements agree on the bits; the step is temporal_ref's ----------------------------------------------------------------
@pytest.mark.parametrize("size", [(3, 2), (11, 7)])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_vectorised_equals_scalar_on_the_bits(T, size):
    cams, frames, state0, moment0, cam0 = _sequence(size, T)
    W, H = size
    for m in (0, 1):
        for demodulate in (True, False):
            for state, moment, cam_prev in ((None, None, None), (state0, moment0, cam0)):
                kw = dict(m=m, demodulate=demodulate)
                a = NR.step_moments(*frames[0], cams[0], T, state, moment, cam_prev, **kw)
                b = NR.step_moments_scalar(*frames[0], cams[0], T, state, moment, cam_prev, **kw)
                assert a[2].dtype == b[2].dtype == np.dtype(T) and a[2].shape == (H, W)
                assert TR.same_bits(a[0], b[0]) and TR.same_state(a[1], b[1]) and TR.same_bits(a[2], b[2]), (kw, state is None)
                for radius in (1, 2, 3):
                    for min_len in (1.0, 4.0, 2.5, 100.0):
                        nk = dict(radius=radius, m=m, min_len=min_len, sigma_depth=0.1 if radius != 2 else 0.02)
                        x, y = NR.noise_map(a[1], a[2], T, **nk), NR.noise_map_scalar(a[1], a[2], T, **nk)
                        assert x.dtype == np.dtype(T) and TR.same_bits(x, y), (kw, nk, state is None)
    # the second step of a chain too (the state and the moments a step left, not hand-made ones)
    s1 = NR.step_moments(*frames[0], cams[0], T, state0, moment0, cam0)
    a, b = NR.step_moments(*frames[1], cams[1], T, s1[1], s1[2], cams[0]), NR.step_moments_scalar(*frames[1], cams[1], T, s1[1], s1[2], cams[0])
    assert TR.same_bits(a[0], b[0]) and TR.same_state(a[1], b[1]) and TR.same_bits(a[2], b[2])
    assert TR.same_bits(NR.noise_map(a[1], a[2], T), NR.noise_map_scalar(a[1], a[2], T))


@pytest.mark.parametrize("size", [(3, 2), (37, 23), (70, 40)])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_step_with_moments_leaves_temporal_refs_image_and_state(T, size):
    cams, frames, state0, moment0, cam0 = _sequence(size, T)
    for kw in (dict(), dict(m=0, demodulate=False, gamma=0), dict(m=7, history_max=3.5, min_weight=0.9, sigma_depth=0.002)):
        st, mo, cp = state0, moment0, cam0
        ref_st = state0
        for k in range(3):
            out, st, mo = NR.step_moments(*frames[k], cams[k], T, st, mo, cp, **kw)
            ref_out, ref_st = TR.step(*frames[k], cams[k], T, ref_st, cp, **kw)
            assert TR.same_bits(out, ref_out) and TR.same_state(st, ref_st), (kw, k)
            cp = cams[k]
        a, b = NR.step_moments(*frames[0], cams[0], T, **kw), TR.step(*frames[0], cams[0], T, **kw)
        assert TR.same_bits(a[0], b[0]) and TR.same_state(a[1], b[1])


def test_the_packed_moment_plane_is_the_headers_layout():
    T = np.float32
    M = np.arange(15, dtype=T).reshape(3, 5)
    flat = NR.pack_moment(M, T)
    assert flat.shape == (16,) and flat.nbytes == 64 and NR.moment_elems(3, 5, np.float64) * 8 == 128 and NR.moment_elems(1, 1, T) == 4
    assert flat[3 * 3 + 2] == M[2, 3] and flat[15] == 0
    assert np.array_equal(NR.unpack_moment(flat, 3, 5), M)


# ---- 2. the committed seeds reach every regime ---------------------------------------------------------------------------------------------
REGIMES = ("temporal", "spatial", "reset", "accepted", "cut_top", "cut_bottom", "cut_left", "cut_right", "invalid_neighbour", "sky_covered_pair", "vt_clamped", "invalid_centre")


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_census_of_the_hand_made_sequences(T):
    """the frames of tests/test_gpu_temporal_noise.py: a step on the hand-made state (history lengths 1..24, on both sides of min_len = 4)
    and a first frame (every pixel resets, every history is short) together reach every regime on each of the two larger frames; the
    3 x 2 frame is smaller than the window of every radius"""
    for size in ((70, 40), (64, 36)):
        cams, frames, state0, moment0, cam0 = _sequence(size, T)
        a = NR.census(*frames[0], cams[0], T, state0, moment0, cam0)
        b = NR.census(*frames[0], cams[0], T, None, None, None)
        print(np.dtype(T).name, size, a, b)
        for k in REGIMES:
            assert a[k] + b[k] > 0, (size, k)
        assert a["temporal"] > 0 and a["spatial"] > 0 and a["reset"] > 0 and a["accepted"] > 0 and a["vt_clamped"] > 0
        assert b["temporal"] == 0 and b["accepted"] == 0 and b["reset"] == b["spatial"] > 0
        one = NR.census(*frames[0], cams[0], T, state0, moment0, cam0, noise=dict(min_len=1.0))
        assert one["spatial"] == 0 and one["temporal"] == a["temporal"] + a["spatial"]          # min_len = 1: never spatial
    cams, frames, state0, moment0, cam0 = _sequence((3, 2), T)
    for radius in (1, 2, 3):
        c = NR.census(*frames[0], cams[0], T, None, None, None, noise=dict(radius=radius))
        assert c["frame_smaller_than_window"] == c["spatial"] == 6 and c["cut_top"] and c["cut_bottom"] and c["cut_left"] and c["cut_right"]
    c = NR.census(*_sequence((1, 1), T)[1][0], _sequence((1, 1), T)[0][0], T, None, None, None)
    assert c["spatial"] + c["invalid_centre"] == 1


# ---- 3. constant frames: the moments are the population variance ---------------------------------------------------------------------------
def _constant_frames(T, colours, W=9, H=6, albedo=(0.5, 0.25, 0.75)):
    feat = np.zeros((H, W, 8), T)
    feat[...] = np.array(list(albedo) + [0.0, 0.6, 0.8, 5.0, 1.0], T)
    return [(np.broadcast_to(np.array(c, T), (H, W, 3)).copy(), feat) for c in colours]


def _run_constant(rtw, T, colours, demodulate, **nk):
    frames = _constant_frames(T, colours)
    H, W = frames[0][0].shape[:2]
    cam = TR.make_camera(rtw, T, (0.3, 0.2, 0.5), (0.1, 0.0, -1.0), W, H)
    st = mo = cp = None
    for image, feat in frames:
        _, st, mo = NR.step_moments(image, feat, cam, T, st, mo, cp, history_max=64.0, demodulate=demodulate, gamma=0)
        cp = cam
    e = [DR.prepare(image, feat, T, demodulate)[2][0, 0] for image, feat in frames]
    return st, mo, e, NR.noise_map(st, mo, T, **nk)


@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_constant_frames_hold_the_population_variance(rtw, T, demodulate):
    """n = 7 spatially constant frames (frame k is one colour c_k and one feature vector everywhere, unit normal, full coverage) through
    identical cameras with history_max = 64 >= n: every pixel accepts, every tap of a frame holds the same values, so the tap mixing is a
    weighted mean of a constant and no geometric tolerance enters.  With e_k the (de)modulated colour the step itself uses (values of T,
    taken as exact rationals), y_k = e_k[0] + e_k[1] + e_k[2] exactly, V = mean(y_k^2) - mean(y_k)^2 exactly, u the unit roundoff and
    Y = sum over the channels of max_k |e_k[c]| (>= every |y_k|, every |Lm|; M <= Y^2), to first order in u, constants rounded up:
        a weighted mean of a constant x over <= 4 taps     fl(w*x) per tap, 3 sums above and 3 below, one quotient: 9 u |x|
        len' = lh + 1 and alpha = 1 / len'                lh carries 9 u, the sum u, the quotient u: alpha = (1/k)(1 + 11 u)
        one blend  xh + alpha*(x - xh),  |x|, |xh| <= S    9 u S (xh) + 11 u S (alpha, on |x - xh| / k <= S) + 3 u S (difference, product, sum) = 23 u S;
                                                           the error already in x_prev is carried with a factor 1 - 1/k <= 1
        y2 = y*y                                           two sums, one product: 5 u Y^2 on top of the blend's 23 u Y^2
    so after n frames  |dE[c]| <= 23 n u max|e[c]|,  |dM| <= 28 n u Y^2,  |dLm| <= (23 n + 2) u Y,  |d(Lm*Lm)| <= (46 n + 5) u Y^2, and
        |fl(M - Lm*Lm) - V| <= (74 n + 6) u Y^2            (the difference itself: u Y^2; clamping at +0 only helps, V >= 0)
    asserted as (80 n + 8) u Y^2 with the slack for the neglected second order.  len is n within (11 n) u n.  The map then is
    sqrt(var / len) / max(Lm, 2^-6) of those values: checked against the same expression in binary64 within 8 u relative plus the
    variance's bound propagated through the square root."""
    rng = np.random.default_rng(7)
    n = 7
    colours = rng.uniform(0.05, 0.9, (n, 3))
    st, mo, e, rho = _run_constant(rtw, T, colours, demodulate, min_len=4.0)
    u = float(np.finfo(T).eps) / 2
    ys = [Fraction(float(x[0])) + Fraction(float(x[1])) + Fraction(float(x[2])) for x in e]
    V = sum(y * y for y in ys) / n - (sum(ys) / n) ** 2
    Y = sum(max(abs(float(x[c])) for x in e) for c in range(3))
    bound = (80 * n + 8) * u * Y * Y
    assert float(V) > 100 * bound                           # (the check is not vacuous: the bound is below 1 % of the variance)
    assert np.all(np.abs(st["L"].astype(np.float64) - n) <= 11 * n * u * n)
    with np.errstate(all="ignore"):
        Lm = ((st["E"][..., 0] + st["E"][..., 1]) + st["E"][..., 2])
        var = np.maximum(mo - Lm * Lm, T(0)).astype(np.float64)
    err = float(np.abs(var - float(V)).max())
    print(f"{np.dtype(T).name} demodulate={demodulate}: V = {float(V):.6e}, max |M - Lm^2 - V| = {err / (u * Y * Y):.1f} u Y^2 (bound {(80 * n + 8)} u Y^2)")
    assert err <= bound
    assert np.abs(Lm.astype(np.float64) - float(sum(ys) / n)).max() <= (23 * n + 2) * 1.1 * u * Y
    want = np.sqrt(float(V) / n) / float(sum(ys) / n)
    tol = want * (8 * u + 0.5 * bound / float(V) + (23 * n + 2) * 1.1 * u * Y / float(sum(ys) / n) + 11 * n * u)
    assert np.isfinite(rho).all() and np.abs(rho.astype(np.float64) - want).max() <= tol


@pytest.mark.parametrize("min_len", [1.0, 4.0, 100.0])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_one_colour_for_all_frames_is_exactly_zero_noise(rtw, T, min_len):
    """one colour for all n frames, its channels powers of two that sum to a power of two: a product by a power of two is exact, so every
    weighted mean of the constant IS the constant (numerator = constant * denominator on the bits), every blend adds alpha * 0, M stays
    y*y = Lm*Lm exactly, and the map is +0 on the bits -- through the temporal branch (min_len 1, 4) and the spatial one (min_len 100)."""
    st, mo, e, rho = _run_constant(rtw, T, [(0.5, 0.25, 0.25)] * 5, False, min_len=min_len)
    assert TR.same_bits(rho, np.zeros_like(rho))
    assert TR.same_bits(mo, np.ones_like(mo)) and (st["L"] > 4).all()


# ---- 4. what it buys ------------------------------------------------------------------------------------------------------------------------
def _orbit(O, T, n, step_deg=0.75):
    """n pinhole cameras on frame F's orbit: its lookfrom turned about the y axis in steps of `step_deg` degrees"""
    cams = []
    for v in range(n):
        a = np.deg2rad(step_deg * v)
        x, zc = 13 * np.cos(a) + 3 * np.sin(a), -13 * np.sin(a) + 3 * np.cos(a)
        cams.append(O.default_camera([x, 2, zc], [0, 0, 0], [0, 1, 0], 20, 16 / 9, 0.0, 10, T))
    return cams


def _dolly(O, T, n, step=0.015):
    """n pinhole cameras on frame F's dolly: its lookfrom moved 1.5 % towards the lookat per frame"""
    return [O.default_camera([13 * (1 - step * v), 2 * (1 - step * v), 3 * (1 - step * v)], [0, 0, 0], [0, 1, 0], 20, 16 / 9, 0.0, 10, T) for v in range(n)]


def accumulate_with_moments(oracle, flat, cams, W, H, T, spp=1, noise=None, **params):
    """the witness along a path of oracle renders -> (the last accumulated linear frame, its features, its noise map, the last frame's own image, the last state)"""
    state = moment = prev = out = raw = feat = None
    for v, cam in enumerate(cams):
        raw, _ = oracle.render(flat, cam, W, H, spp, T=T, seed=1 + v, gamma=False)
        feat, poisoned = FR.resolve(FR.items(flat, cam, W, H, spp, 0, 1 + v, T), T)
        assert not poisoned.any()
        out, state, moment = NR.step_moments(np.ascontiguousarray(raw), feat, CamObj(cam), T, state, moment, prev, gamma=0, **params)
        prev = CamObj(cam)
    return out, feat, NR.noise_map(state, moment, T, **(noise or {})), raw, state


@pytest.mark.parametrize("path", ["orbit", "dolly"])
def test_the_guided_filter_behind_the_map_helps(oracle, path):
    """DESIGN.md 7.18's orbit and dolly over frame F's scene at 64 x 36, 1 spp, 8 frames, everything at its defaults, linear, against a
    1024-spp oracle render of the last camera: the accumulated frame, the accumulated frame behind the plain filter at its defaults, and the
    accumulated frame behind the guided filter (sigma_color at the guided default) with the new map.  All three are finite; the condition is
    MSE(guided) < MSE(frame 8's own 1-spp image), strictly, test_it_helps_along_an_orbit's.  The three ratios are printed (DESIGN.md 7.19's
    record); whether guided beats plain is recorded there, not asserted."""
    T = np.float32
    flat = FR.frame_f(T)[0]
    W, H = 64, 36
    cams = (_orbit if path == "orbit" else _dolly)(oracle, T, 8)
    t0 = time.time()
    acc, feat, rho, raw, state = accumulate_with_moments(oracle, flat, cams, W, H, T)
    truth, _ = oracle.render(flat, cams[-1], W, H, 1024, T=T, seed=99, gamma=False)
    truth = truth.astype(np.float64)
    plain = DR.denoise(acc, feat, T, gamma=0)
    guided = AR.guided(acc, feat, rho, T, gamma=0, **{k: v for k, v in AR.GUIDED_DEFAULTS.items() if k != "gamma"})
    assert np.isfinite(acc).all() and np.isfinite(plain).all() and np.isfinite(guided).all() and np.isfinite(rho).all()
    mse = lambda x: float(((x.astype(np.float64) - truth) ** 2).mean())
    m_raw, m_acc, m_plain, m_guided = mse(raw), mse(acc), mse(plain), mse(guided)
    short = float((state["L"] < 4).mean())
    print(f"{path}: MSE frame 8 at 1 spp {m_raw:.6f}; ratios accumulated {m_acc / m_raw:.3f}  plain {m_plain / m_raw:.3f}  guided {m_guided / m_raw:.3f}; "
          f"median rho {float(np.median(rho)):.3f}, pixels with len < min_len {100 * short:.1f} %  ({time.time() - t0:.1f} s)")
    assert m_guided < m_raw
