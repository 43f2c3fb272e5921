"""The witness of the wide-aperture stage (tests/wide_aperture_ref.py; include/rtw_hip.h rtw_wide_aperture_*) on the CPU: it agrees with
itself (vectorised against scalar, on the bits, the image and every workspace region), its hand-made cases reach every regime the GPU test
relies on, max_radius <= 8 is the defocus stage, a closed aperture is the identity, an impulse on a flat wide frame keeps its sum, sharp
foreground stays sharp in front of a background at R = 16, and a pinhole frame given a wide aperture is closer to the lens-sampled truth
than the defocus stage at its clamp leaves it.  No GPU."""
import functools
import time

import numpy as np
import pytest

import defocus_ref as FO
import features_ref as FR
import wide_aperture_ref as WA
from conftest import CamObj
from test_defocus_ref import _flat_frame

PRECISIONS = [np.float32, np.float64]


@functools.lru_cache(maxsize=None)
def _cases(size, T):
    W, H = size
    return WA.handmade_cases(H, W, T, WA.SEEDS[T])


# ---- 1. the witness agrees with itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", WA.CPU_SIZES)
@pytest.mark.parametrize("T", PRECISIONS)
def test_vectorised_equals_scalar_on_the_bits(T, size):
    """the image and every region of the workspace, of every hand-made case"""
    for k, c in enumerate(_cases(size, T)):
        args = (c["image"], c["features"], c["cam"], T)
        vec, sca = WA.wide_aperture(*args, **c["params"]), WA.wide_aperture_scalar(*args, **c["params"])
        assert set(vec[1]) == set(WA.REGIONS)
        assert WA.same_result(vec, sca), (size, k, [n for n in vec[1] if not WA.same_bits(vec[1][n], sca[1][n])])


@pytest.mark.parametrize("T", PRECISIONS)
def test_census_of_the_hand_made_cases(T):
    """over the cases of the CPU frame sizes together, every regime on at least 16 pixels, blocks or taps (a condition: the seeds are
    picked so that it holds); the GPU test's other sizes run the same generator"""
    total = dict.fromkeys(WA.REGIMES, 0)
    for size in WA.CPU_SIZES:
        for k, c in enumerate(_cases(size, T)):
            cen = WA.census(c, T)
            print(np.dtype(T).name, size, "case", k, {r: v for r, v in cen.items() if v})
            for r in WA.REGIMES:
                total[r] += cen[r]
    print(np.dtype(T).name, "total", total)
    assert all(total[r] >= 16 for r in WA.REGIMES), {r: v for r, v in total.items() if v < 16}


def test_the_layout_is_the_sum_of_its_regions():
    """every region begins on a multiple of four elements, in the header's order; max_radius <= 8: the defocus stage's workspace; monotone"""
    for W, H in WA.SIZES + [(1920, 1080)]:
        for mr in (1, 8):
            assert WA.work_elems(H, W, mr) == FO.work_elems(H, W)
        for mr in (9, 16, 17, 32):
            regions, total = WA.layout(H, W, mr)
            assert list(regions) == list(WA.REGIONS) and total % 4 == 0
            ends = 0
            for at, count, shape in regions.values():
                assert at % 4 == 0 and at >= ends and count == int(np.prod(shape))
                ends = at + count
            assert total >= ends and regions["coc"][0] == FO.work_elems(H, W)
    for mr in (9, 17):
        for n in range(1, 70):
            assert WA.work_elems(7, n, mr) <= WA.work_elems(7, n + 1, mr) and WA.work_elems(n, 7, mr) <= WA.work_elems(n + 1, 7, mr)


# ---- 2. what it is on simple frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", PRECISIONS)
def test_max_radius_up_to_8_is_the_defocus_stage_on_the_bits(T):
    """both witnesses of this stage against both witnesses of that one, on that stage's own hand-made cases (max_radius 1 .. 8)"""
    for c in FO.handmade_cases(17, 33, T, FO.SEEDS[T])[3:]:
        args = (c["image"], c["features"], c["cam"], T)
        ref = FO.defocus(*args, **c["params"])
        assert FO.same_defocus(WA.wide_aperture(*args, **c["params"]), ref) and set(ref[1]) == {"coc", "tile"}
        assert FO.same_defocus(WA.wide_aperture_scalar(*args, **c["params"]), ref)


@pytest.mark.parametrize("size", WA.CPU_SIZES)
@pytest.mark.parametrize("T", PRECISIONS)
def test_a_closed_aperture_is_the_identity_on_the_bits(T, size):
    """lens_radius = 0: K = 0, every radius is 0, t = 0 everywhere and the narrow stage passes through -- the input on the bits; NaN where
    not valid"""
    for c in _cases(size, T)[:6]:
        out, work = WA.wide_aperture(c["image"], c["features"], c["cam"], T, lens_radius=0.0, focus_dist=c["params"]["focus_dist"], max_radius=c["params"]["max_radius"])
        valid = ~np.isnan(work["coc"][..., 1])
        assert valid.any() and (~valid).any() and (work["tile"] <= 0).all() and (work["lo_tile"] <= 0).all()          # (0, or -1: a one-pixel tile that is not valid)
        assert WA.same_bits(out[valid], c["image"][valid]) and np.isnan(out[~valid]).all()


@pytest.mark.parametrize("T", PRECISIONS)
def test_an_impulse_on_a_flat_wide_frame_keeps_its_sum(T):
    """A white pixel on a black wall far behind the focus plane, K = 40, max_radius 12: every pixel of the 60 x 60 frame sits at the clamp,
    R = 12, so t = 1 and out = U everywhere; s = 2, every block has R_s = 6 and one depth.  Reduce leaves 1/4 in one small pixel (exact).
    The small gather runs with m = 6, n_g = 13*13 = 169 taps, every window within 6 + 6 small pixels of the impulse inside the 30 x 30 small
    frame: by the argument of the defocus stage's impulse test the small image O sums to (1/4)(1 + theta), |theta| <= n_g u.  Compose: the
    four weights of a pixel are dyadic and sum to 1 exactly, so ws = 1 and U = acc; acc is four products (one rounding each) and three
    additions of non-negative terms, relative error <= 4u; and every small pixel away from the border receives a total weight of s^2 = 4
    from the full-size pixels.  So the output sums to 1 within (n_g + 4)u + O(u^2): asserted with n = 174, u = eps / 2."""
    H = W = 60
    cam = FO.handmade_camera(H, W, T)
    lr = FO.lens_for(cam, T, W, T(40))
    feat = _flat_frame(cam, T, H, W, np.full(W, 400.0))
    image = np.zeros((H, W, 3), T)
    image[30, 30] = 1
    out, work = WA.wide_aperture(image, feat, cam, T, lens_radius=lr, max_radius=12)
    assert (work["coc"][..., 0] == 12).all() and (work["lo_coc"][..., 0] == 6).all() and work["lo_image"][15, 15, 0] == T(0.25)
    lit = np.argwhere(out[..., 0] > 0)
    assert lit.min() >= 2 * (15 - 6) - 1 and lit.max() <= 2 * (15 + 6) + 2 and (out[..., 0] == out[..., 2]).all()
    n = 174
    total = float(out[..., 0].astype(np.float64).sum())
    print(np.dtype(T).name, "sum of the spread impulse", total, "lit pixels", len(lit))
    assert abs(total - 1.0) <= n * (np.finfo(T).eps / 2)


@pytest.mark.parametrize("T", PRECISIONS)
def test_sharp_foreground_stays_sharp_over_a_background_at_16_px(T):
    """Columns 0 .. 11 at the focus plane (R = 0 < 4/2: t = 0, out = N, and N is the input there by the defocus stage's own argument), the
    others far behind it at the clamp R = 16: the foreground equals the input on the bits although every small block along the edge mixes
    both; the background is the wide result, t = 1"""
    H, W = 20, 24
    cam = FO.handmade_camera(H, W, T)
    lr = FO.lens_for(cam, T, W, T(40))
    rng = np.random.default_rng(5)
    image = rng.uniform(0.0, 2.0, size=(H, W, 3)).astype(T)
    feat = _flat_frame(cam, T, H, W, np.where(np.arange(W) < 12, 4.0, 400.0))
    d = {}
    out, work = WA.wide_aperture(image, feat, cam, T, lens_radius=lr, max_radius=16, details=d)
    fg = np.broadcast_to(np.arange(W) < 12, (H, W))
    assert (work["coc"][..., 0][fg] < 0.5).all() and (work["coc"][..., 0][~fg] == 16).all() and (d["t"][~fg] == 1).all()
    assert WA.same_bits(out[fg], image[fg])
    assert (WA.bits(out[~fg]) != WA.bits(image[~fg])).mean() > 0.9 and (WA.bits(out[~fg]) != WA.bits(work["narrow"][~fg])).mean() > 0.9


# ---- 3. it helps -----------------------------------------------------------------------------------------------------------------------------------
def test_it_is_closer_to_the_lens_sampled_truth_than_the_clamp_at_8(oracle):
    """scene_random_spheres(seed 1), binary32, 192 x 108, lookfrom (13, 2, 3) -> (0, 0, 0), vfov 20, focus 10, aperture 1.2 (K = 18.37 px).
    Truth: the oracle's own lens-sampled render at 512 spp.  Strictly: the MSE to the truth of the pinhole frame under this stage is below
    that under the defocus stage at its clamp of 8, over the whole frame and over the pixels with R > 8, for a 64-spp and for a 4-spp input
    (features: the feature witness at min(spp, 16) samples), for max_radius 16 and for max_radius 32; and the noise floor (the MSE between
    two independent truths) is below every gap on the R > 8 rows.  The figures are printed."""
    T = np.float32
    W, H, APERTURE = 192, 108, 1.2
    t0 = time.time()
    scene = oracle.scene_random_spheres(1, T)
    lens = oracle.default_camera([13, 2, 3], [0, 0, 0], [0, 1, 0], 20, 16 / 9, APERTURE, 10, T)
    pin = oracle.default_camera([13, 2, 3], [0, 0, 0], [0, 1, 0], 20, 16 / 9, 0.0, 10, T)
    truth_a = oracle.render(scene, lens, W, H, 512, T=T, seed=1000, gamma=False)[0].astype(np.float64)
    truth_b = oracle.render(scene, lens, W, H, 512, T=T, seed=2000, gamma=False)[0].astype(np.float64)
    floor = float(((truth_a - truth_b) ** 2).mean())
    camo = CamObj(pin)
    rows = []
    for spp in (64, 4):
        sharp = np.ascontiguousarray(oracle.render(scene, pin, W, H, spp, T=T, seed=7, gamma=False)[0])
        feat, poisoned = FR.resolve(FR.items(scene, pin, W, H, min(spp, 16), 0, 7, T), T)
        assert not poisoned.any()
        narrow = FO.defocus(sharp, feat, camo, T, lens_radius=APERTURE / 2, max_radius=8)[0]
        lensed = oracle.render(scene, lens, W, H, spp, T=T, seed=7, gamma=False)[0]
        for mr in (16, 32):
            soft, work = WA.wide_aperture(sharp, feat, camo, T, lens_radius=APERTURE / 2, max_radius=mr)
            assert np.isfinite(soft).all() and WA.same_bits(work["narrow"], narrow)
            wide = work["coc"][..., 0] > 8
            everything = np.ones((H, W), bool)
            mse = lambda a, m: float(((a.astype(np.float64) - truth_a) ** 2)[m].mean())
            for name, m in (("whole frame", everything), ("R > 8", wide)):
                a, b = mse(narrow, m), mse(soft, m)
                rows.append((spp, mr, name, a, b))
                print(f"{spp:3d} spp, max_radius {mr}: {name:12s} ({int(m.sum())} px) MSE sharp {mse(sharp, m):.6f}  clamp 8 {a:.6f}  wide {b:.6f} (x {b / a:.3f})  "
                      f"lens-sampled at the same spp {mse(lensed, m):.6f}")
    print(f"noise floor (two independent truths): {floor:.6f}  ({time.time() - t0:.1f} s)")
    for spp, mr, name, a, b in rows:
        assert b < a, (spp, mr, name, a, b)
        if name == "R > 8":
            assert floor < a - b, (spp, mr, floor, a - b)
