"""The witness of temporal reuse over moving spheres (tests/motion_ref.py; include/rtw_hip.h rtw_motion_table_*, rtw_first_hit_motion_*,
rtw_animated_step_*) on the CPU: it agrees with itself (vectorised against scalar), with the static witnesses where nothing moves, with the
geometry where camera and surface move together, with the table's rules, and it helps where spheres move.  No GPU."""
import time

import numpy as np
import pytest

import features_ref as FR
import motion_ref as MR
import temporal_clamp_ref as CR
import temporal_noise_ref as NR
import temporal_ref as TR
from conftest import CamObj
from test_temporal_ref import _plain_frame, orbit

PRECISIONS = [np.float32, np.float64]


def _steps(size, T):
    W, H = size
    return MR.handmade_steps(H, W, T, MR.SEEDS[T])


# ---- 1. the witness agrees with itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", TR.SIZES)
@pytest.mark.parametrize("T", PRECISIONS)
def test_vectorised_equals_scalar_on_the_bits(T, size):
    """every step of the hand-made sequence with its hand-made motion plane: plain, with moments, and (up to 37 x 23) clamped with guides"""
    for s in _steps(size, T):
        a = (s["image"], s["features"], s["cam"], T, s["motion"], s["state"], s["cam_prev"])
        assert MR.same_step(MR.step(*a), MR.step_scalar(*a))
        assert MR.same_step(MR.step(*a, s["moment"]), MR.step_scalar(*a, s["moment"]))
        if size[0] * size[1] <= 37 * 23:
            ck = dict(radius=1, guides=True, sigma=1.0, len_scale=0.5)
            assert MR.same_step(MR.step(*a, s["moment"], clamp=ck, m=0, demodulate=False, gamma=0), MR.step_scalar(*a, s["moment"], clamp=ck, m=0, demodulate=False, gamma=0))


@pytest.mark.parametrize("size", MR.SIZES)
@pytest.mark.parametrize("T", PRECISIONS)
def test_zero_motion_is_the_static_step_on_the_bits(T, size):
    """x - 0 == x: the plain step, the step with moments and the clamped step with moments, image, state and moment plane; so is the first frame"""
    for s in _steps(size, T):
        zero = np.zeros_like(s["motion"])
        a = (s["image"], s["features"], s["cam"], T)
        out, nxt, M = MR.step(*a, zero, s["state"], s["cam_prev"])
        ref = TR.step(*a, s["state"], s["cam_prev"])
        assert M is None and TR.same_bits(out, ref[0]) and TR.same_state(nxt, ref[1])
        ref = NR.step_moments(*a, s["state"], s["moment"], s["cam_prev"])
        assert MR.same_step(MR.step(*a, zero, s["state"], s["cam_prev"], s["moment"]), ref[:3])
        for ck in (dict(radius=1, guides=False, sigma=1.0, len_scale=0.5), dict(radius=3, guides=True, sigma=0.5, len_scale=1.0)):
            assert MR.same_step(MR.step(*a, zero, s["state"], s["cam_prev"], s["moment"], clamp=ck), CR.step_clamped(*a, s["state"], s["cam_prev"], s["moment"], clamp=ck))
        first = MR.step(*a)
        assert TR.same_bits(first[0], TR.step(*a)[0]) and TR.same_state(first[1], TR.step(*a)[1])


@pytest.mark.parametrize("T", PRECISIONS)
def test_a_nan_slot_resets_exactly_its_pixel(T):
    """one non-finite component in the slot of an accepted covered pixel: that pixel resets (e' = e, len' = 1), every other pixel keeps its
    bits; the fourth element and the slot of a pixel that is not covered change nothing at all"""
    s = _steps((37, 23), T)[0]
    a = (s["image"], s["features"], s["cam"], T)
    zero = np.zeros_like(s["motion"])
    d = {}
    ref = MR.step(*a, zero, s["state"], s["cam_prev"], s["moment"], details=d)
    cand = np.argwhere(d["valid"] & d["has"] & d["accept"])
    assert len(cand) >= 3
    for (i, j), bad in zip(cand[[0, len(cand) // 2, -1]], (np.nan, np.inf, -np.inf)):
        mv = zero.copy()
        mv[i, j, 1] = bad
        got = MR.step(*a, mv, s["state"], s["cam_prev"], s["moment"])
        assert got[1]["L"][i, j] == 1 and not TR.same_bits(got[1]["E"][i, j], ref[1]["E"][i, j])
        others = np.ones(d["valid"].shape, bool)
        others[i, j] = False
        assert TR.same_bits(got[0][others], ref[0][others]) and TR.same_bits(got[2][others], ref[2][others])
        assert all(TR.same_bits(got[1][k][others], ref[1][k][others]) for k in ("E", "G", "L"))
    mv = zero.copy()
    mv[..., 3] = np.nan
    mv[~d["has"], 0:3] = np.nan
    assert MR.same_step(MR.step(*a, mv, s["state"], s["cam_prev"], s["moment"]), ref)


@pytest.mark.parametrize("size", [(37, 23), (70, 41)])
@pytest.mark.parametrize("T", PRECISIONS)
def test_camera_and_surface_moved_together_reproject_every_pixel_onto_itself(rtw, T, size):
    """the camera translates by v and every surface moves by the same v: every covered pixel's point lay where it is seen now, (x, y) = (j, i),
    within the bound test_identical_cameras_reproject_every_pixel_onto_itself uses -- temporal_ref.geometry_bound plus the two roundings the
    motion adds to d (the subtraction of m and the origin's own shift: 2 u (|o| + |v|) / z_min per component, far below the bound's slack, so the
    bound itself is asserted) and 2^-8 pixel in binary64.  A sky pixel ignores the motion: the cameras do not turn, so it too stays."""
    W, H = size
    v = np.array([0.375, -0.25, 0.5])
    prev = TR.make_camera(rtw, T, (0.3, 0.2, 0.5), (0.1, 0.0, -1.0), W, H)
    cam = TR.make_camera(rtw, T, (0.3, 0.2, 0.5), (0.1, 0.0, -1.0), W, H)
    cam.origin = (np.asarray(prev.origin, np.float64) + v).astype(T)
    cam.lower_left_corner = (np.asarray(prev.lower_left_corner, np.float64) + v).astype(T)
    image, feat = _plain_frame(H, W, T, np.random.default_rng(3))
    mv = np.zeros((H, W, 4), T)
    mv[..., 0:3] = v.astype(T)
    d = {}
    MR.step(image, feat, cam, T, mv, TR.step(image, feat, prev, T)[1], prev, details=d)
    ex = np.abs(d["x"].astype(np.float64) - np.arange(W)[None, :]).max()
    ey = np.abs(d["y"].astype(np.float64) - np.arange(H)[:, None]).max()
    bx, by = TR.geometry_bound(cam, W, H, T, z_min=1.0)
    print(f"{np.dtype(T).name} {W}x{H}: max |x - j| = {ex:.3e} (bound {bx:.3e}), max |y - i| = {ey:.3e} (bound {by:.3e})")
    assert d["front"].all() and d["inr"].all()
    assert ex <= bx and ey <= by
    if T is np.float64:
        assert ex <= 2.0 ** -8 and ey <= 2.0 ** -8
    assert d["accept"].sum() > 0.5 * W * H


# ---- 2. the table and the pass ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_table_rules(oracle, T):
    """one subtraction in T per component; a sphere the previous scene lacks and a sphere whose radius changed (by one ulp) get three NaNs;
    the fourth element is 0"""
    prev = {k: (np.asarray(v).copy() if isinstance(v, np.ndarray) else v) for k, v in FR.frame_f(T)[0].items()}
    cur = {k: (np.asarray(v).copy() if isinstance(v, np.ndarray) else v) for k, v in prev.items()}
    n = int(cur["n"])
    rng = np.random.default_rng(2)
    for k in ("cx", "cy", "cz"):
        cur[k] = (cur[k].astype(np.float64) + rng.uniform(-0.3, 0.3, n)).astype(T)
    cur["r"][7] = np.nextafter(cur["r"][7], T(np.inf))
    prev = {k: (v[:n - 2] if isinstance(v, np.ndarray) else n - 2) for k, v in prev.items()}
    tab = MR.motion_table(prev, cur, T)
    assert tab.dtype == T and tab.shape == (n, 4) and (tab[:, 3] == 0).all()
    changed = np.zeros(n, bool)
    changed[[7, n - 2, n - 1]] = True
    assert np.isnan(tab[changed, 0:3]).all() and np.isfinite(tab[~changed]).all()
    for c, k in enumerate(("cx", "cy", "cz")):
        ref = cur[k][:n - 2] - prev[k]
        assert ref.dtype == T and TR.same_bits(tab[:n - 2, c][~changed[:n - 2]], ref[~changed[:n - 2]])


def test_the_pass_names_the_lower_index_among_equal_hits(oracle):
    """two identical spheres at indices a < b: every pixel that sees them carries a; the oracle's own loop (the later sphere wins) says b"""
    import rtw_oracle as O
    T = np.float32
    flat = dict(n=4, cx=np.array([0, 0, 0, 2], T), cy=np.array([-100.5, 0, 0, 0], T), cz=np.array([-1, -1, -1, -1], T), r=np.array([100, 0.5, 0.5, 0.5], T),
                kind=np.zeros(4, np.int32), ar=np.full(4, 0.5, T), ag=np.full(4, 0.5, T), ab=np.full(4, 0.5, T), param=np.zeros(4, T))
    cam = O.default_camera([0, 0, 1], [0, 0, -1], [0, 1, 0], 60, 16 / 9, 0.0, 2, T)
    tab = np.zeros((4, 4), T)
    tab[:, 0] = [10, 11, 12, 13]
    plane = MR.motion_pass(flat, cam, 32, 18, T, tab)
    ids = plane[..., 3]
    assert (ids == 1).any() and not (ids == 2).any() and (ids == -1).any() and (ids == 0).any() and (ids == 3).any()
    assert (plane[ids == 1, 0] == 11).all() and (plane[ids == -1, 0:3] == 0).all()
    late, _ = O.hit_world_batch(flat, MR.centre_rays(cam, 32, 18, T).reshape(-1, 6), 1e-4, np.inf, T)
    assert ((late.reshape(18, 32) == 2) == (ids == 1)).all()
    assert (MR.motion_pass(flat, cam, 32, 18, T)[..., 0:3] == 0).all()


# ---- 3. the hand-made motion planes reach what the GPU test relies on ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", MR.SIZES)
@pytest.mark.parametrize("T", PRECISIONS)
def test_census_of_the_hand_made_motion(T, size):
    """every step of every frame of H*W >= 12: an accepted pixel whose first tap differs from the zero-motion one, a pixel reset by a
    non-finite slot, a pixel the motion step accepts and the plain step resets, and one of the converse kind"""
    W, H = size
    for k, s in enumerate(_steps(size, T)):
        c = MR.census(s["image"], s["features"], s["cam"], T, s["motion"], s["state"], s["cam_prev"])
        print(np.dtype(T).name, size, "step", k, c)
        if H * W >= 12:
            assert c["moved_accepted"] >= 1 and c["nan_reset"] >= 1 and c["gained"] >= 1 and c["lost"] >= 1, (size, k, c)
        assert np.isnan(s["motion"][..., 3]).any()          # (the fourth element is arbitrary: it has no effect)


# ---- 4. it helps ----------------------------------------------------------------------------------------------------------------------------------
def animated_scenes(T, n_frames, speed=1.0):
    """frame F's scene with three rolling radius-1 spheres and 60 drifting small ones -> (list of flat scenes, the moving indices)"""
    base = FR.frame_f(T)[0]
    n = int(base["n"])
    r = np.asarray(base["r"], np.float64)
    big = np.flatnonzero(r == 1.0)
    assert len(big) == 3
    small = np.array([k for k in range(1, n) if r[k] != 1.0])
    rng = np.random.default_rng(5)
    pick = rng.choice(small, 60, replace=False)
    dx, dz = np.zeros(n), np.zeros(n)
    dx[big] = (0.24, -0.18, 0.15)
    dx[pick] = rng.uniform(-0.15, 0.15, 60)
    dz[pick] = rng.uniform(-0.15, 0.15, 60)
    scenes = []
    for v in range(n_frames):
        s = {k: (np.asarray(a).copy() if isinstance(a, np.ndarray) else a) for k, a in base.items()}
        s["cx"] = (np.asarray(base["cx"], np.float64) + speed * v * dx).astype(T)
        s["cz"] = (np.asarray(base["cz"], np.float64) + speed * v * dz).astype(T)
        scenes.append(s)
    return scenes, np.concatenate([big, pick])


def accumulate_animation(oracle, scenes, cams, W, H, T, motion, spp=1):
    """the witness along oracle renders of a moving scene -> (the last accumulated linear frame, the last frame's own image, the mean history
    length per pixel, the ids of the last two frames)"""
    state = prev = out = raw = None
    ids = []
    for v, (flat, cam) in enumerate(zip(scenes, cams)):
        raw, _ = oracle.render(flat, cam, W, H, spp, T=T, seed=1 + v, gamma=False)
        feat, poisoned = FR.resolve(FR.items(flat, cam, W, H, spp, 0, 1 + v, T), T)
        assert not poisoned.any()
        plane = MR.motion_pass(flat, cam, W, H, T, MR.motion_table(scenes[v - 1], flat, T) if v else None)
        ids.append(plane[..., 3].astype(np.int64))
        mv = None if v == 0 else (plane if motion else np.zeros_like(plane))
        out, state, _ = MR.step(np.ascontiguousarray(raw), feat, CamObj(cam), T, mv, state, prev, gamma=0)
        prev = CamObj(cam)
    return out, raw, state["L"], ids[-2:]


def test_it_helps_where_spheres_move(oracle):
    """frame F's scene, 64 x 36, 8 frames at 1 spp, defaults, linear, a fixed pinhole camera, truth at 512 spp; three big spheres roll and 60
    small ones drift.  Strictly: on the moving pixels (a centre-ray id of frame 7 or 6 names a moving sphere) the motion step beats the
    plain step and the frame alone; over the whole frame it beats the plain step.  The ratios are printed."""
    T = np.float32
    W, H, N = 64, 36, 8
    t0 = time.time()
    scenes, moving = animated_scenes(T, N)
    cams = [orbit(oracle, T, 1)[0]] * N
    out_m, raw, len_m, ids = accumulate_animation(oracle, scenes, cams, W, H, T, True)
    out_p, _, len_p, _ = accumulate_animation(oracle, scenes, cams, W, H, T, False)
    truth, _ = oracle.render(scenes[-1], cams[-1], W, H, 512, T=T, seed=99, gamma=False)
    assert np.isfinite(out_m).all() and np.isfinite(out_p).all()
    mask = np.isin(ids[0], moving) | np.isin(ids[1], moving)
    truth = truth.astype(np.float64)
    mse = lambda a, m: float(((a.astype(np.float64) - truth) ** 2)[m].mean())
    everything = np.ones((H, W), bool)
    r = {k: (mse(a, mask), mse(a, everything)) for k, a in (("frame alone", raw), ("plain step", out_p), ("motion step", out_m))}
    print(f"moving pixels: {int(mask.sum())}; mean history length there: plain {float(len_p[mask].mean()):.2f}, motion {float(len_m[mask].mean()):.2f}")
    for k, (a, b) in r.items():
        print(f"{k:12s} MSE moving pixels {a:.5f}  whole frame {b:.5f}")
    print(f"ratios on the moving pixels: motion / plain {r['motion step'][0] / r['plain step'][0]:.3f}, motion / frame {r['motion step'][0] / r['frame alone'][0]:.3f}; "
          f"whole frame motion / plain {r['motion step'][1] / r['plain step'][1]:.3f}  ({time.time() - t0:.1f} s)")
    assert mask.sum() > 100
    assert r["motion step"][0] < r["plain step"][0]
    assert r["motion step"][0] < r["frame alone"][0]
    assert r["motion step"][1] < r["plain step"][1]
