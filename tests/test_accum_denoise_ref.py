"""The witness of the accumulator side of the denoiser (tests/accum_denoise_ref.py) against itself, against expectations worked out by
hand and against the CPU oracle, no GPU: the vectorised guided filter equals the scalar one on the bits; a map of ones reproduces the
plain witness where the brightness is constant; a low noise estimate keeps detail that a high one removes; the noise map on hand-made
words; and on an adaptive render made of oracle samples the guided filter at its default lowers the error against a 1024-spp render."""
import numpy as np
import pytest

import accum_denoise_ref as AR
import accum_words as AW
import denoise_ref as DR
import features_ref as FR
from conftest import load_golden

SEEDS = {np.float32: 11, np.float64: 12}


@pytest.mark.parametrize("m", [0, 1])
@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_vectorised_equals_scalar_on_the_bits(T, levels, m):
    image, feat = DR.handmade(11, 7, T, SEEDS[T])
    noise = AR.special_noise(11, 7, T, SEEDS[T] + 100)
    assert noise.dtype == np.dtype(T) and noise[0, 0] == 0 and np.isnan(noise).sum() == 1 and np.isinf(noise).sum() == 1
    assert (noise == T(2.0 ** -30)).sum() == 1 and (noise == T(3.0e25)).sum() == 1
    for demodulate, gamma in ((True, 1), (False, 0)):
        a = AR.guided(image, feat, noise, T, levels=levels, m=m, demodulate=demodulate, gamma=gamma)
        b = AR.guided_scalar(image, feat, noise, T, levels=levels, m=m, demodulate=demodulate, gamma=gamma)
        assert a.dtype == b.dtype == np.dtype(T)
        assert DR.same_bits(a, b), (levels, m, demodulate, gamma)
        # a pixel whose noise entry is not finite is not valid
        assert np.isnan(a[~np.isfinite(noise)]).all() and np.isfinite(a).any()
        assert not DR.same_bits(a, DR.denoise(image, feat, T, levels=levels, m=m, demodulate=demodulate, gamma=gamma))
    # the clamps: a tiny and a huge entry give V_MIN and V_MAX
    v = AR.guided_prepare(image, feat, noise, T, True)[7]
    ok = np.isfinite(image).all(axis=2) & np.isfinite(feat).all(axis=2)
    assert (v[ok & (noise == T(2.0 ** -30))] == T(AR.V_MIN)).all() and (v[ok & (noise == T(3.0e25))] == T(AR.V_MAX)).all()
    assert (v[ok & (noise == 0)] == T(AR.V_MIN)).all()


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_map_of_ones_is_the_plain_filter_where_the_brightness_is_constant(T):
    """every pixel has (e0 + e1) + e2 = 1/2 exactly, so with rho = 1: s = 1/2, v = 1/4 and dc / v = 4 dc exactly; with sigma_color doubled
    inv_sc is a quarter, exactly: (4 dc)(inv_sc / 4) = dc inv_sc -- the plain witness, on the bits"""
    rng = np.random.default_rng(3)
    _, feat = DR.handmade(11, 7, T, SEEDS[T])
    d = rng.integers(-64, 65, size=(11, 7)) * 2.0 ** -10
    image = np.stack([0.25 + d, 0.125 - d, np.full((11, 7), 0.125)], axis=2).astype(T)
    assert ((image[..., 0] + image[..., 1]) + image[..., 2] == T(0.5)).all()
    image[2, 3, 1] = np.nan
    ones = np.ones((11, 7), T)
    for levels in (1, 3):
        a = AR.guided(image, feat, ones, T, levels=levels, sigma_color=1.0, demodulate=False, gamma=0)
        b = DR.denoise(image, feat, T, levels=levels, sigma_color=0.5, demodulate=False, gamma=0)
        assert DR.same_bits(a, b), levels
        assert np.isnan(a).any() and not DR.same_bits(a, AR.guided(image, feat, ones, T, levels=levels, sigma_color=0.5, demodulate=False, gamma=0))


def _checker_frame(T):
    H, W = 16, 32
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sign = np.where((ii + jj) & 1, 1.0, -1.0)
    image = (0.5 + 0.02 * sign)[..., None] * np.ones(3)
    feat = np.concatenate([np.ones((H, W, 3)), np.zeros((H, W, 2)), np.ones((H, W, 1)), np.full((H, W, 1), 5.0), np.ones((H, W, 1))], axis=2)
    noise = np.where(jj < W // 2, 2.0 ** -10, 1.0)
    return image.astype(T), feat.astype(T), noise.astype(T)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_low_noise_estimate_keeps_what_a_high_one_removes(T):
    """the same checker of amplitude 0.02 in both halves, uniform guides; the map says `noise-free' on the left and `noisy' on the right"""
    image, feat, noise = _checker_frame(T)
    amp = lambda x, cols: float(np.abs(x[:, cols].astype(np.float64) - 0.5).mean())
    left, right = slice(0, 10), slice(22, 32)                     # away from the border between the halves (3 levels reach 4 + 2 + 1 ... pixels)
    g = AR.guided(image, feat, noise, T, gamma=0)
    u = DR.denoise(image, feat, T, gamma=0)
    assert np.isfinite(g).all() and np.isfinite(u).all()
    a0 = amp(image, left)
    assert abs(a0 - 0.02) < 1e-6 and abs(amp(image, right) - 0.02) < 1e-6
    assert amp(g, left) > amp(u, left)                            # guided keeps strictly more of the checker on the left than the plain filter
    assert a0 - amp(g, right) > a0 - amp(g, left)                 # ... and removes strictly more on the right than on the left
    assert amp(g, left) > 0.9 * a0 and amp(g, right) < 0.1 * a0   # (by a wide margin)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_noise_map_on_hand_made_words(T):
    names = set()
    for name, words, floor, expect in AR.noise_cases():
        got = AR.noise_map(words, AR.NCHUNKS, AR.NW, AR.NH, AR.NSPP, AR.NCS, floor, T)
        assert got.dtype == np.dtype(T) and got.shape == (AR.NH, AR.NW)
        for (i, j), want in expect.items():
            if want is None:
                assert np.isnan(got[i, j]), (name, i, j)
            else:
                assert got[i, j] == np.dtype(T).type(want), (name, i, j, got[i, j], want)
        assert np.isnan(got).sum() == int((words[..., 6] != 0).sum()), name
        names.add(name)
    assert {"negative_h_in_the_corner", "h_most_negative", "floor_0_and_y_0", "poisoned_centre_and_neighbour",
            "tiles_with_different_chunk_counts", "ragged_last_tile_row"} <= names
    # the samples of a tile: min(spp, C_t * chunk_spp)
    assert sorted(set(AW.tile_divisors(AR.NCHUNKS, AR.NW, AR.NH, AR.NSPP, AR.NCS).reshape(-1))) == [6, 12, 18, 20]


# ---- the quality condition --------------------------------------------------------------------------------------
W48, H27, SPP, DEPTH, SEED, CHECKS, FLOOR = 48, 27, 64, 8, 7, [16, 32, 48], 0.03


def adaptive_case48(oracle):
    """cfg2's scene at 48 x 27, 64 chunks of one sample, checkpoints 16 / 32 / 48: the adaptive accumulator the rule makes of the ORACLE's
    samples (tolerance: the middle of the gap between two tiles' D / M ratios that splits the tiles most evenly into stopping first, in
    between and never, as tests/test_gpu_adaptive.py picks it), its tile-prefix features, and a 1024-spp render of the frame"""
    from rtw_amd import reference_decisions
    T = np.float32
    g = load_golden("cfg2_random_320x180_64spp_d16_f32", numerics="reference")
    samples = np.empty((H27, W48, SPP, 3), np.float64)
    for i in range(H27):
        for j in range(W48):
            samples[i, j] = oracle.pixel_samples(g["flat"], g["cam"], W48, H27, SPP, i + 1, j + 1, T=T, max_depth=DEPTH, seed=SEED, n_chunks=SPP)
    words_at = AR.oracle_words(samples, 1, CHECKS + [SPP])
    ratios = {}
    for c in CHECKS:
        _, D, _, M = reference_decisions(words_at[c], W48, H27, c, 1.0, FLOOR, return_terms=True)
        ratios[c] = np.array([d / m for d, m in zip(D, M)])
    allr = np.sort(np.unique(np.concatenate(list(ratios.values()))))
    tol, best = None, -1
    for lo, hi in zip(allr[:-1], allr[1:]):
        cand = 0.5 * (lo + hi)
        if min(abs(allr - cand) / cand) <= 1e-6:
            continue
        first = ratios[16] <= cand
        never = np.all([ratios[c] > cand for c in CHECKS], axis=0)
        score = min(first.sum(), never.sum(), (~first & ~never).sum())
        if score > best:
            tol, best = cand, score
    ct = AR.rule_chunks(words_at, CHECKS, SPP, 1, W48, H27, tol, FLOOR)
    words = AR.adaptive_words(words_at, ct, W48, H27)
    raw = AW.resolve(words, AW.tile_divisors(ct, W48, H27, SPP, 1), 0, T)
    prev = oracle.set_numerics("reference")
    try:
        it = FR.items(g["flat"], g["cam"], W48, H27, SPP, SPP, SEED, T, key="cfg2_48x27")
        truth, _ = oracle.render(g["flat"], g["cam"], W48, H27, 1024, T=T, max_depth=DEPTH, seed=SEED + 1, gamma=False)
    finally:
        oracle.set_numerics(prev)
    feat = AR.tile_prefix_features(it, T, ct, W48, H27)
    return dict(T=T, chunks=ct, words=words, raw=np.ascontiguousarray(raw), feat=feat, truth=truth.astype(np.float64), tol=float(tol))


def test_quality_of_the_guided_filter_on_the_oracle(oracle):
    """The condition is MSE(guided at its default) < MSE(unfiltered adaptive image), linear space, against 1024 spp.  The figures
    are printed; guided against plain is reported in DESIGN.md 7.11, not asserted."""
    cs = adaptive_case48(oracle)
    T = cs["T"]
    assert len(set(int(c) for c in cs["chunks"])) >= 3                      # tiles stopped at several checkpoints
    noise = AR.noise_map(cs["words"], cs["chunks"], W48, H27, SPP, 1, FLOOR, T)
    mse = lambda x: float(((x.astype(np.float64) - cs["truth"]) ** 2).mean())
    out = AR.guided(cs["raw"], cs["feat"], noise, T, gamma=0, **{k: v for k, v in AR.GUIDED_DEFAULTS.items() if k != "gamma"})
    plain = DR.denoise(cs["raw"], cs["feat"], T, gamma=0)
    assert np.isfinite(out).all()
    print(f"MSE raw {mse(cs['raw']):.6e}  guided {mse(out):.6e}  plain at its default {mse(plain):.6e}")
    assert mse(out) < mse(cs["raw"])
    import importlib
    assert importlib.import_module("rtw_amd.denoise").GUIDED_SIGMA_COLOR == AR.GUIDED_DEFAULTS["sigma_color"]
