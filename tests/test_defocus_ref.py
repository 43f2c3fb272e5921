"""The witness of the defocus stage (tests/defocus_ref.py; include/rtw_hip.h rtw_defocus_*) on the CPU: it agrees with itself (vectorised
against scalar, on the bits), its hand-made cases reach every regime the GPU test relies on, a closed aperture is the identity, an impulse
spreads into a disc that keeps its sum, sharp foreground stays sharp in front of a blurred background, a focus override is a camera rebuilt
with that focus, and a defocused pinhole frame is closer to the lens-sampled truth than the sharp one.  No GPU."""
import functools
import time

import numpy as np
import pytest

import defocus_ref as FO
import features_ref as FR
from conftest import CamObj

PRECISIONS = [np.float32, np.float64]
CPU_SIZES = [(17, 33), (33, 17)]


@functools.lru_cache(maxsize=None)
def _cases(size, T):
    W, H = size
    return FO.handmade_cases(H, W, T, FO.SEEDS[T])


# ---- 1. the witness agrees with itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", CPU_SIZES)
@pytest.mark.parametrize("T", PRECISIONS)
def test_vectorised_equals_scalar_on_the_bits(T, size):
    """the image, the CoC plane and the tile plane of every hand-made case"""
    for k, c in enumerate(_cases(size, T)):
        args = (c["image"], c["features"], c["cam"], T)
        assert FO.same_defocus(FO.defocus(*args, **c["params"]), FO.defocus_scalar(*args, **c["params"])), (size, k)


@pytest.mark.parametrize("T", PRECISIONS)
def test_census_of_the_hand_made_cases(T):
    """over the cases of the two CPU frame sizes together, every regime on at least 16 pixels or taps (a condition: the seeds are picked so
    that it holds); the GPU test's other sizes run the same generator"""
    total = dict.fromkeys(FO.REGIMES, 0)
    for size in CPU_SIZES:
        for k, c in enumerate(_cases(size, T)):
            cen = FO.census(c, T)
            print(np.dtype(T).name, size, "case", k, {r: v for r, v in cen.items() if v})
            for r in FO.REGIMES:
                total[r] += cen[r]
    print(np.dtype(T).name, "total", total)
    assert all(total[r] >= 16 for r in FO.REGIMES), {r: v for r, v in total.items() if v < 16}


# ---- 2. what it is on simple frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", CPU_SIZES)
@pytest.mark.parametrize("T", PRECISIONS)
def test_a_closed_aperture_is_the_identity_on_the_bits(T, size):
    """lens_radius = 0: K = 0, every radius is 0, every tile passes through -- the input on the bits; NaN where not valid"""
    for c in _cases(size, T)[3:8]:
        out, work = FO.defocus(c["image"], c["features"], c["cam"], T, lens_radius=0.0, focus_dist=c["params"]["focus_dist"], max_radius=c["params"]["max_radius"])
        valid = ~np.isnan(work["coc"][..., 1])
        assert valid.any() and (~valid).any() and (work["tile"] == 0).all()
        assert FO.same_bits(out[valid], c["image"][valid]) and np.isnan(out[~valid]).all()


def _flat_frame(cam, T, H, W, zax_of_column):
    """full coverage, every pixel at the axial depth zax_of_column[j]: feature 6 is the distance along the pixel's own ray"""
    import motion_ref as MR
    rays = MR.centre_rays(cam, W, H, T).astype(np.float64)
    ca = -(rays[..., 3:6] @ np.asarray(cam.w, np.float64))
    feat = np.zeros((H, W, 8), T)
    feat[..., 0:3], feat[..., 5], feat[..., 7] = 0.5, 1.0, 1.0
    feat[..., 6] = (np.asarray(zax_of_column, np.float64)[None, :] / ca).astype(T)
    return feat


@pytest.mark.parametrize("T", PRECISIONS)
def test_an_impulse_spreads_into_a_disc_that_keeps_its_sum(T):
    """A white pixel at axial depth 1 in front of a black wall at depth 400, the focus plane at 4, K = 12, max_radius 3: both sit at the clamp,
    R = 3, so every pixel of the 15 x 15 frame gathers with the same set of (cover, w) pairs.  The impulse lands exactly on the pixels closer
    than R + 1/2 = 3.5 to it.  Its sum is preserved: with n = 49 taps, a_d = fl(cover_d*w) and S their exact sum, wsum_X = S(1 + delta),
    |delta| <= (n - 1)u (recursive summation of positive terms), out_X = fl(a_X / wsum_X) = (a_X / S)(1 + theta), |theta| <= n u + O(u^2); the
    a_X over the disc are the a_d over the window, so sum_X out_X = 1 + at most n u relative.  Asserted with 2 n u, u = eps / 2."""
    H = W = 15
    cam = FO.handmade_camera(H, W, T)
    lr = FO.lens_for(cam, T, W, T(12))
    feat = _flat_frame(cam, T, H, W, np.full(W, 400.0))
    feat[7, 7, 6] = _flat_frame(cam, T, H, W, np.full(W, 1.0))[7, 7, 6]
    image = np.zeros((H, W, 3), T)
    image[7, 7] = 1
    d = {}
    out, work = FO.defocus(image, feat, cam, T, lens_radius=lr, max_radius=3, details=d)
    assert (work["coc"][..., 0] == 3).all() and work["coc"][7, 7, 1] < work["coc"][0, 0, 1]
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dist = np.sqrt((ii - 7.0) ** 2 + (jj - 7.0) ** 2)
    assert np.array_equal(out[..., 0] > 0, dist < 3.5) and (out[..., 0] == out[..., 1]).all()
    n = 49
    total = float(out[..., 0].astype(np.float64).sum())
    print(np.dtype(T).name, "sum of the spread impulse", total, "lit pixels", int((out[..., 0] > 0).sum()))
    assert abs(total - 1.0) <= 2 * n * (np.finfo(T).eps / 2)
    assert FO.same_defocus((out, work), FO.defocus_scalar(image, feat, cam, T, lens_radius=lr, max_radius=3))


@pytest.mark.parametrize("T", PRECISIONS)
def test_sharp_foreground_stays_sharp_over_a_blurred_background(T):
    """Columns 0 .. 11 at the focus plane (R = 0, Rh = 1/2, w = 4), the others far behind it (R at the clamp): for a foreground pixel X every
    tap behind it is limited to X's own circle, Re = 1/2, and covers nothing at dist >= 1 -- out = (4c)/4 = c on the bits; the background
    next to the edge does change"""
    H, W = 20, 24
    cam = FO.handmade_camera(H, W, T)
    lr = FO.lens_for(cam, T, W, T(12))
    rng = np.random.default_rng(5)
    image = rng.uniform(0.0, 2.0, size=(H, W, 3)).astype(T)
    zax = np.where(np.arange(W) < 12, 4.0, 400.0)
    feat = _flat_frame(cam, T, H, W, zax)
    d = {}
    out, work = FO.defocus(image, feat, cam, T, lens_radius=lr, max_radius=8, details=d)
    fg = np.broadcast_to(np.arange(W) < 12, (H, W))
    assert (work["coc"][..., 0][fg] < 0.5).all() and (work["coc"][..., 0][~fg] == 8).all() and d["lim_true"] > 0
    assert FO.same_bits(out[fg], image[fg])
    assert (FO.bits(out[~fg]) != FO.bits(image[~fg])).mean() > 0.9


@pytest.mark.parametrize("T", PRECISIONS)
def test_a_focus_override_is_a_camera_rebuilt_with_that_focus(T):
    """K does not move with the override (it is measured on the camera's own focus plane), so focus_dist = 2f with lens_radius r equals the
    camera rebuilt with its focus plane at 2f -- horizontal, vertical and llc - origin doubled, the same rays on the bits -- and lens_radius 2r"""
    W, H = 33, 17
    c = _cases((W, H), T)[9]
    cam, cam2 = FO.handmade_camera(H, W, T, focus=4.0, origin=(0, 0, 0)), FO.handmade_camera(H, W, T, focus=8.0, origin=(0, 0, 0))     # (origin 0: doubling is exact)
    for k in ("horizontal", "vertical"):
        setattr(cam2, k, (getattr(cam, k) * T(2)).astype(T))
    cam2.lower_left_corner = (cam2.origin - cam2.horizontal / T(2) - cam2.vertical / T(2) - T(8) * cam2.w).astype(T)
    p = dict(c["params"], focus_dist=0.0)
    a = FO.defocus(c["image"], c["features"], cam, T, **dict(p, focus_dist=8.0))
    b = FO.defocus(c["image"], c["features"], cam2, T, **dict(p, lens_radius=2 * p["lens_radius"]))
    assert FO.same_defocus(a, b) and (a[1]["tile"] >= 0.5).any()
    assert not FO.same_bits(a[0], FO.defocus(c["image"], c["features"], cam, T, **p)[0])


# ---- 3. it helps -----------------------------------------------------------------------------------------------------------------------------------
def test_it_brings_a_pinhole_frame_closer_to_the_lens_sampled_truth(oracle):
    """scene_random_spheres(seed 1), binary32, 128 x 72, lookfrom (13, 2, 3) -> (0, 0, 0), vfov 20, focus 10, aperture 0.6, max_radius 8.
    Truth: the oracle's own lens-sampled render at 256 spp.  Strictly: the defocused pinhole frame's MSE to the truth is below the sharp
    pinhole frame's, over the whole frame and over the pixels with R > 1, for a 256-spp and for a 4-spp input (features: the feature
    witness at min(spp, 16) samples); at 4 spp it is also below the MSE of the lens-sampled render at 4 spp; and the noise floor (the MSE
    between two independent truths) is below the gap asserted on the 256-spp rows.  The ratios are printed."""
    T = np.float32
    W, H, APERTURE = 128, 72, 0.6
    t0 = time.time()
    scene = oracle.scene_random_spheres(1, T)
    lens = oracle.default_camera([13, 2, 3], [0, 0, 0], [0, 1, 0], 20, 16 / 9, APERTURE, 10, T)
    pin = oracle.default_camera([13, 2, 3], [0, 0, 0], [0, 1, 0], 20, 16 / 9, 0.0, 10, T)
    truth_a = oracle.render(scene, lens, W, H, 256, T=T, seed=1000, gamma=False)[0].astype(np.float64)
    truth_b = oracle.render(scene, lens, W, H, 256, T=T, seed=2000, gamma=False)[0].astype(np.float64)
    floor = float(((truth_a - truth_b) ** 2).mean())
    camo = CamObj(pin)
    rows = {}
    for spp in (256, 4):
        sharp = np.ascontiguousarray(oracle.render(scene, pin, W, H, spp, T=T, seed=7, gamma=False)[0])
        feat, poisoned = FR.resolve(FR.items(scene, pin, W, H, min(spp, 16), 0, 7, T), T)
        assert not poisoned.any()
        soft, work = FO.defocus(sharp, feat, camo, T, lens_radius=APERTURE / 2, max_radius=8)
        assert np.isfinite(soft).all()
        wide = work["coc"][..., 0] > 1
        everything = np.ones((H, W), bool)
        mse = lambda a, m: float(((a.astype(np.float64) - truth_a) ** 2)[m].mean())
        lensed = oracle.render(scene, lens, W, H, spp, T=T, seed=7, gamma=False)[0]
        rows[spp] = [(mse(sharp, m), mse(soft, m), mse(lensed, m)) for m in (everything, wide)]
        print(f"{spp} spp: largest R {float(work['coc'][..., 0].max()):.2f} px, {int(wide.sum())} pixels with R > 1, {int((work['coc'][..., 0] >= 8).sum())} at the clamp")
        for name, (a, b, c) in zip(("whole frame", "R > 1"), rows[spp]):
            print(f"  {name:12s} MSE sharp {a:.6f}  defocused {b:.6f} (x {b / a:.3f})  lens-sampled at the same spp {c:.6f}")
    print(f"noise floor (two independent truths): {floor:.6f}  ({time.time() - t0:.1f} s)")
    for spp in (256, 4):
        for a, b, _ in rows[spp]:
            assert b < a
    assert rows[4][0][1] < rows[4][0][2]
    assert all(floor < a - b for a, b, _ in rows[256])
