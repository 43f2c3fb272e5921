"""The denoiser's witness (tests/denoise_ref.py) against itself and against the CPU oracle, no GPU: the vectorised restatement equals the
scalar one on the bits; the hand-made frames hold every regime of the definition; an edge in albedo and normal is not crossed; and on a
real 4-spp render the filter lowers the error against a 1024-spp render."""
import numpy as np
import pytest

import denoise_ref as DR
import features_ref as FR

SEEDS = {np.float32: 11, np.float64: 12}


@pytest.mark.parametrize("m", [0, 1, 7])
@pytest.mark.parametrize("levels", [1, 2, 3, 4])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_vectorised_equals_scalar_on_the_bits(T, levels, m):
    image, feat = DR.handmade(11, 7, T, SEEDS[T])
    for demodulate, gamma in ((True, 1), (False, 0)):
        a = DR.denoise(image, feat, T, levels=levels, m=m, demodulate=demodulate, gamma=gamma)
        b = DR.denoise_scalar(image, feat, T, levels=levels, m=m, demodulate=demodulate, gamma=gamma)
        assert a.dtype == b.dtype == np.dtype(T)
        assert DR.same_bits(a, b), (levels, m, demodulate, gamma)
        assert np.isnan(a).any() and np.isfinite(a).any()


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(11, 7), (37, 23), (70, 41)])
def test_census_of_the_hand_made_frames(T, shape):
    """a weakened generator fails here"""
    image, feat = DR.handmade(shape[0], shape[1], T, SEEDS[T])
    assert image.dtype == feat.dtype == np.dtype(T) and image.shape == shape + (3,) and feat.shape == shape + (8,)
    c = DR.census(image, feat)
    assert c["cov0"] >= 3 and c["cov_frac"] >= 3 and c["cov1"] >= 3, c
    assert c["tiny_albedo"] >= 3 and c["z_le_0"] >= 2, c
    assert c["non_finite"] >= 3 and c["non_finite_border"] >= 1, c


def test_the_filter_changes_the_image_and_the_parameters_matter():
    T = np.float32
    image, feat = DR.handmade(11, 7, T, SEEDS[T])
    base = DR.denoise(image, feat, T, gamma=0)
    valid = ~np.isnan(base).any(axis=2)
    assert not np.array_equal(base[valid], image[valid])
    for kw in (dict(levels=2), dict(m=3), dict(sigma_color=0.25), dict(sigma_depth=0.5), dict(demodulate=False)):
        assert not DR.same_bits(DR.denoise(image, feat, T, gamma=0, **kw), base), kw
    g = DR.denoise(image, feat, T, gamma=1)
    assert DR.same_bits(g, np.sqrt(base))


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_step_in_albedo_and_normal_is_not_crossed(T):
    """|out - clean| <= max |noisy - clean| on each side of the step: no pixel moves towards the other side by more than its own side's noise"""
    noisy, clean, feat = DR.step_frame(T, 5)
    H, W = noisy.shape[:2]
    for demodulate in (True, False):
        out = DR.denoise(noisy, feat, T, levels=3, demodulate=demodulate, gamma=0)
        assert np.isfinite(out).all()
        for side in (slice(0, W // 2), slice(W // 2, W)):
            bound = np.abs(noisy[:, side] - clean[:, side]).max()
            assert np.abs(out[:, side] - clean[:, side]).max() <= bound, (demodulate, side)
        # ... and the filter did something: the error went down on the whole
        assert np.abs(out - clean).mean() < 0.6 * np.abs(noisy - clean).mean()


def test_quality_on_the_oracle(oracle):
    """frame F's scene and camera at 64 x 36, 4 spp in 4 chunks, against a 1024-spp oracle render; defaults, linear.
    The condition is MSE(denoised) < MSE(raw); the ratio is printed."""
    T = np.float32
    flat, cam, _, _ = FR.frame_f(T)
    W, H = 64, 36
    raw, _ = oracle.render(flat, cam, W, H, 4, T=T, seed=1, n_chunks=4, gamma=False)
    truth, _ = oracle.render(flat, cam, W, H, 1024, T=T, seed=2, gamma=False)
    feat, poisoned = FR.resolve(FR.items(flat, cam, W, H, 4, 4, 1, T), T)
    assert not poisoned.any()
    out = DR.denoise(np.ascontiguousarray(raw), feat, T, gamma=0)
    assert np.isfinite(out).all()
    truth = truth.astype(np.float64)
    mse_raw = float(((raw.astype(np.float64) - truth) ** 2).mean())
    mse_out = float(((out.astype(np.float64) - truth) ** 2).mean())
    print(f"MSE raw {mse_raw:.6f}  denoised {mse_out:.6f}  ratio {mse_out / mse_raw:.3f}")
    assert mse_out < mse_raw
