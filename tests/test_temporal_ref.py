"""The temporal reprojection's witness (tests/temporal_ref.py) against itself, against geometry and against the CPU oracle, no GPU: the
vectorised restatement equals the scalar one on the bits; the committed seeds reach every branch of the definition; the reprojection is
geometrically right (identity for identical cameras, the analytic parallax for a translated one) within a derived rounding bound; a step in
normal is not crossed; and along a real 1-spp camera path the accumulated frame is closer to a 1024-spp render than the frame itself."""
import functools
import time

import numpy as np
import pytest

import denoise_ref as DR
import features_ref as FR
import temporal_ref as TR
from conftest import CamObj


@functools.lru_cache(maxsize=None)
def _sequence(size, T):
    W, H = size
    return TR.handmade_sequence(H, W, T, TR.SEEDS[T], 3)


# ---- 1. the two restatements agree on the bits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, 1, 7])
@pytest.mark.parametrize("size", [(5, 3), (37, 23)])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_vectorised_equals_scalar_on_the_bits(T, size, m):
    cams, frames, state0, cam0 = _sequence(size, T)
    for demodulate in (True, False):
        for gamma in (0, 1):
            for state, cam_prev in ((None, None), (state0, cam0)):
                kw = dict(m=m, demodulate=demodulate, gamma=gamma)
                a = TR.step(*frames[0], cams[0], T, state, cam_prev, **kw)
                b = TR.step_scalar(*frames[0], cams[0], T, state, cam_prev, **kw)
                assert a[0].dtype == b[0].dtype == np.dtype(T)
                assert TR.same_bits(a[0], b[0]) and TR.same_state(a[1], b[1]), (kw, state is None)
                assert all(a[1][k].dtype == np.dtype(T) for k in "EGL")
                assert np.isfinite(a[0]).any() and (np.isnan(a[0]).any() or size[0] * size[1] < 12)
    # the second step of the chain too (the state a step left, not a hand-made one)
    s1 = TR.step(*frames[0], cams[0], T, state0, cam0, m=m)[1]
    a, b = TR.step(*frames[1], cams[1], T, s1, cams[0], m=m), TR.step_scalar(*frames[1], cams[1], T, s1, cams[0], m=m)
    assert TR.same_bits(a[0], b[0]) and TR.same_state(a[1], b[1])


def test_the_packed_state_is_the_headers_layout():
    T = np.float32
    cams, frames, state0, cam0 = _sequence((5, 3), T)
    flat = TR.pack_state(state0, T)
    assert flat.shape == (TR.state_elems(3, 5, T),) and flat.nbytes == 544 and TR.state_elems(3, 5, np.float64) * 8 == 1088
    i, j, n = 2, 3, 15
    p = j * 3 + i
    assert TR.same_bits(flat[4 * p:4 * p + 4], state0["E"][i, j]) and TR.same_bits(flat[4 * n + 4 * p:4 * n + 4 * p + 4], state0["G"][i, j])
    assert flat[8 * n + p] == state0["L"][i, j]
    assert TR.same_state(TR.unpack_state(flat, 3, 5), state0)


# ---- 2. the committed seeds reach every branch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(37, 23), (70, 41)])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_census_of_the_hand_made_sequences(T, size):
    """a weakened generator fails here: every count is of step 0 (on the hand-made previous state), the step the GPU comparison sweeps"""
    cams, frames, state0, cam0 = _sequence(size, T)
    c = TR.census(*frames[0], cams[0], T, state0, cam0)
    for key in ("accepted", "reset_not_front", "reset_not_inr", "reset_low_weight", "fewer_than_4_inside", "tap_not_valid", "sky_from_sky", "sky_hit_mismatch",
                "len_saturated", "non_finite"):
        assert c[key] >= 1, (key, c)
    # the later steps of the chain still blend and still reset
    state, cam_prev = state0, cam0
    for k in range(3):
        ck = TR.census(*frames[k], cams[k], T, state, cam_prev)
        assert ck["accepted"] >= 1 and ck["reset_not_inr"] >= 1 and ck["reset_low_weight"] >= 1 and ck["non_finite"] >= 1, (k, ck)
        state, cam_prev = TR.step(*frames[k], cams[k], T, state, cam_prev)[1], cams[k]
    assert (state["L"] > 3).any()


def test_the_parameters_matter():
    T = np.float32
    cams, frames, state0, cam0 = _sequence((37, 23), T)
    base = TR.step(*frames[0], cams[0], T, state0, cam0)
    for kw in (dict(m=3), dict(sigma_depth=0.002), dict(min_weight=0.9), dict(min_weight=2.0 ** -20), dict(history_max=1.0), dict(history_max=3.5), dict(demodulate=False)):
        got = TR.step(*frames[0], cams[0], T, state0, cam0, **kw)
        assert not (TR.same_bits(got[0], base[0]) and TR.same_state(got[1], base[1])), kw
    g0 = TR.step(*frames[0], cams[0], T, state0, cam0, gamma=0)
    assert TR.same_bits(base[0], np.sqrt(g0[0])) and TR.same_state(base[1], g0[1])          # gamma touches the image alone
    # history_max = 1: len stays 1 and alpha = 1, so every pixel keeps its own colour -- up to the two roundings of eh + (e - eh),
    # u (|e - eh| + |e|) <= 3 u times the largest magnitude involved
    one = TR.step(*frames[0], cams[0], T, state0, cam0, history_max=1.0, demodulate=False, gamma=0)
    valid = ~np.isnan(one[0]).any(axis=2)
    mag = max(float(np.abs(frames[0][0][valid]).max()), float(np.abs(state0["E"][..., 0:3]).max()))
    assert (one[1]["L"][valid] == 1).all()
    assert np.abs(one[0][valid].astype(np.float64) - frames[0][0][valid]).max() <= 3 * (np.finfo(T).eps / 2) * mag


# ---- 3. geometry ------------------------------------------------------------------------------------------------------------------------------
def _plain_frame(H, W, T, rng, z_lo=1.0, z_hi=20.0):
    """finite everywhere: coverage 0 or 1, depths in [z_lo, z_hi]"""
    cov = (rng.random((H, W)) < 0.7).astype(np.float64)
    feat = np.concatenate([rng.uniform(0.1, 1, (H, W, 3)), np.array([0.0, 0.0, 1.0]) * cov[..., None], (rng.uniform(z_lo, z_hi, (H, W)) * cov)[..., None], cov[..., None]], axis=2)
    return rng.uniform(0, 1, (H, W, 3)).astype(T), feat.astype(T)


@pytest.mark.parametrize("size", [(37, 23), (70, 41)])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_identical_cameras_reproject_every_pixel_onto_itself(rtw, T, size):
    """a pinhole camera and cam_prev == cam: (x, y) = (j, i).  binary64: within 2^-8 pixel.  binary32: within temporal_ref.geometry_bound,
    derived from the operation count ("Temporal reprojection") -- about 140 u W for this camera, 5.8e-4 pixel at 70 wide (measured: 1.5e-5)."""
    W, H = size
    cam = TR.make_camera(rtw, T, (0.3, 0.2, 0.5), (0.1, 0.0, -1.0), W, H)
    image, feat = _plain_frame(H, W, T, np.random.default_rng(3))
    d = {}
    TR.step(image, feat, cam, T, TR.step(image, feat, cam, T)[1], cam, details=d)
    ex = np.abs(d["x"].astype(np.float64) - np.arange(W)[None, :]).max()
    ey = np.abs(d["y"].astype(np.float64) - np.arange(H)[:, None]).max()
    bx, by = TR.geometry_bound(cam, W, H, T, z_min=1.0)
    print(f"{np.dtype(T).name} {W}x{H}: max |x - j| = {ex:.3e} (bound {bx:.3e}), max |y - i| = {ey:.3e} (bound {by:.3e})")
    assert d["front"].all() and d["inr"].all()
    assert ex <= bx and ey <= by
    assert bx < 2.0 ** -8 and by < 2.0 ** -8              # (both precisions stay below the binary64 criterion at these sizes)
    if T is np.float64:
        assert ex <= 2.0 ** -8 and ey <= 2.0 ** -8
    # every covered pixel with an accepted history keeps the depth it projects to: zexp is its own z
    assert d["accept"].sum() > 0.5 * W * H


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_translated_camera_shifts_a_plane_by_the_analytic_parallax(rtw, T):
    """the camera moves along its u by delta past a plane that faces it at distance Z: every pixel of the plane lay f*delta / (Z*h) of the
    viewport's width -- W*f*delta / (Z*h) pixels -- further right in the previous frame, rows unchanged; within the same bound"""
    W, H, Z, delta = 70, 41, 6.0, 0.375
    prev = TR.make_camera(rtw, T, (0.3, 0.2, 0.5), (0.1, 0.0, -1.0), W, H)
    o64, u64 = np.asarray(prev.origin, np.float64), np.asarray(prev.u, np.float64)
    cam = TR.make_camera(rtw, T, (0.3, 0.2, 0.5), (0.1, 0.0, -1.0), W, H)
    cam.origin = (o64 + delta * u64).astype(T)
    cam.lower_left_corner = (np.asarray(prev.lower_left_corner, np.float64) + delta * u64).astype(T)
    # the plane's Euclidean depth per pixel, in binary64 from the moved camera's own fields: Z * |D| / (-D.w)
    o, llc, hor, ver, w = (np.asarray(getattr(cam, k), np.float64) for k in ("origin", "lower_left_corner", "horizontal", "vertical", "w"))
    su = (np.arange(W) + 1.5) / W
    tv = (H - np.arange(H) - 0.5) / H
    D = (llc - o)[None, None, :] + su[None, :, None] * hor + tv[:, None, None] * ver
    depth = Z * np.linalg.norm(D, axis=2) / -(D @ w)
    feat = np.concatenate([np.full((H, W, 3), 0.5), np.broadcast_to(w, (H, W, 3)), depth[..., None], np.ones((H, W, 1))], axis=2).astype(T)
    image = np.full((H, W, 3), 0.25, T)
    d = {}
    TR.step(image, feat, cam, T, TR.step(image, feat, prev, T)[1], prev, details=d)
    h, f = np.linalg.norm(hor), -float(TR._dot64(llc - o, w))
    d_eff = float(TR._dot64(np.asarray(cam.origin, np.float64) - o64, hor / h))
    shift = W * f * d_eff / (Z * h)
    assert 1.0 < shift < 3.0
    ex = np.abs(d["x"].astype(np.float64) - (np.arange(W)[None, :] + shift)).max()
    ey = np.abs(d["y"].astype(np.float64) - np.arange(H)[:, None]).max()
    bx, by = TR.geometry_bound(cam, W, H, T, z_min=Z)
    print(f"{np.dtype(T).name}: parallax {shift:.6f} px, max error x {ex:.3e} (bound {bx:.3e}), y {ey:.3e} (bound {by:.3e})")
    assert ex <= bx and ey <= by
    # the columns whose history left the frame reset, the others are accepted with the plane's own depth
    inside = np.arange(W) + shift < W
    assert d["inr"][:, inside].all() and not d["inr"][:, ~inside].any() and (~inside).sum() >= 1
    assert d["accept"][:, np.arange(W) + shift < W - 1].all()


# ---- 4. a step is not crossed ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, 1])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_step_in_normal_is_not_crossed(rtw, T, m):
    """denoise_ref.step_frame (orthogonal normals left and right of column W/2), identical cameras, a previous state with colours of its own
    on each side, min_weight small: the normals' dot product across the step is exactly 0, so a tap of the other side has weight 0 and
    every accumulated colour is a convex combination of its own side's values -- the previous state's and the frame's.  It lies within their
    range, widened by 16 u times the largest magnitude: the blend is 4 products and 3 sums per sum, two quotients, a difference, a product
    and a sum -- fewer than 16 roundings, each relative to a value no larger than the range's largest magnitude."""
    noisy, clean, feat = DR.step_frame(T, 5)
    H, W = noisy.shape[:2]
    cam = TR.make_camera(rtw, T, (0.3, 0.2, 0.5), (0.1, 0.0, -1.0), W, H)
    rng = np.random.default_rng(17)
    prev = TR.step(noisy, feat, cam, T, demodulate=False, gamma=0)[1]
    left = np.arange(W) < W // 2
    prev["E"][..., 0:3] = np.where(left[None, :, None], rng.uniform(2.0, 2.5, (H, W, 3)), rng.uniform(-1.5, -1.0, (H, W, 3))).astype(T)
    prev["L"][...] = rng.integers(1, 6, (H, W)).astype(T)
    d = {}
    out, nxt = TR.step(noisy, feat, cam, T, prev, cam, m=m, min_weight=2.0 ** -10, demodulate=False, gamma=0, details=d)
    assert d["accept"].all() and np.isfinite(out).all()
    assert TR.same_bits(out, nxt["E"][..., 0:3])
    u = np.finfo(T).eps / 2
    for side in (left, ~left):
        for k in range(3):
            vals = np.concatenate([prev["E"][:, side, k].ravel(), noisy[:, side, k].ravel()]).astype(np.float64)
            lo, hi, mag = vals.min(), vals.max(), np.abs(vals).max()
            got = out[:, side, k].astype(np.float64)
            assert got.min() >= lo - 16 * u * mag and got.max() <= hi + 16 * u * mag, (k, got.min(), got.max(), lo, hi)
    # channel 0: the two sides' ranges are disjoint, so is the result; and the history was used
    assert out[:, left, 0].min() > out[:, ~left, 0].max() + 0.25
    assert not np.array_equal(out, noisy)
    assert (nxt["L"] >= 2).all()


# ---- 5. it helps ------------------------------------------------------------------------------------------------------------------------------------
def orbit(O, T, n, step_deg=0.75):
    """n pinhole cameras on frame F's orbit: its lookfrom turned about the y axis in steps of `step_deg` degrees"""
    cams = []
    for v in range(n):
        a = np.deg2rad(step_deg * v)
        x, zc = 13 * np.cos(a) + 3 * np.sin(a), -13 * np.sin(a) + 3 * np.cos(a)
        cams.append(O.default_camera([x, 2, zc], [0, 0, 0], [0, 1, 0], 20, 16 / 9, 0.0, 10, T))
    return cams


def accumulate(oracle, flat, cams, W, H, T, spp=1, **params):
    """the witness along a path of oracle renders at `spp` -> (the last accumulated linear frame, the last frame's own linear image)"""
    state, prev, out, raw = None, None, None, None
    for v, cam in enumerate(cams):
        raw, _ = oracle.render(flat, cam, W, H, spp, T=T, seed=1 + v, gamma=False)
        feat, poisoned = FR.resolve(FR.items(flat, cam, W, H, spp, 0, 1 + v, T), T)
        assert not poisoned.any()
        out, state = TR.step(np.ascontiguousarray(raw), feat, CamObj(cam), T, state, prev, gamma=0, **params)
        prev = CamObj(cam)
    return out, raw


def test_it_helps_along_an_orbit(oracle):
    """8 pinhole cameras on an orbit over frame F's scene at 64 x 36, 1 spp each, defaults, linear: frame 8 accumulated by the witness
    against a 1024-spp oracle render of camera 8.  The condition is MSE(accumulated) < MSE(frame 8's own 1-spp image), strictly; the ratio
    is printed."""
    T = np.float32
    flat = FR.frame_f(T)[0]
    W, H = 64, 36
    cams = orbit(oracle, T, 8)
    t0 = time.time()
    out, raw = accumulate(oracle, flat, cams, W, H, T)
    truth, _ = oracle.render(flat, cams[-1], W, H, 1024, T=T, seed=99, gamma=False)
    assert np.isfinite(out).all()
    truth = truth.astype(np.float64)
    mse_raw = float(((raw.astype(np.float64) - truth) ** 2).mean())
    mse_out = float(((out.astype(np.float64) - truth) ** 2).mean())
    print(f"MSE frame 8 at 1 spp {mse_raw:.6f}  accumulated {mse_out:.6f}  ratio {mse_out / mse_raw:.3f}  ({time.time() - t0:.1f} s)")
    assert mse_out < mse_raw
