"""The witness of the present stage (tests/present_ref.py) on the CPU: with the defaults it is imageio.to_u8 on the bits -- on random frames,
on special values and on real rounding ties --, the dither matrix is the Bayer matrix the header quotes, and the flags act as defined."""
import numpy as np
import pytest

import present_ref as PR


@pytest.fixture(scope="module")
def to_u8(rtw):
    return rtw.imageio.to_u8


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_witness_with_defaults_is_to_u8_on_random_frames(to_u8, T):
    rng = np.random.default_rng(5)
    for H, W in ((1, 1), (7, 5), (54, 96)):
        img = rng.uniform(-0.25, 1.25, (H, W, 3)).astype(T)
        got = PR.present(img)
        assert got.dtype == np.uint8 and got.shape == (H, W, 3) and got.flags.c_contiguous
        assert np.array_equal(got, to_u8(img))
    assert got.min() == 0 and got.max() == 255


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_witness_with_defaults_is_to_u8_on_special_values(to_u8, T):
    vals = PR.special_values(T)
    assert vals.dtype == T and np.isnan(vals).sum() == 6 and np.isinf(vals).sum() == 2 and (vals == 0).sum() == 2
    img = PR.as_frame(vals, T, 5)
    got = PR.present(img)
    with np.errstate(invalid="ignore"):                                    # (widening a signalling NaN raises the flag)
        assert np.array_equal(got, to_u8(img))
    flat = dict(zip(vals[:30].tolist(), got.reshape(-1)[:30].tolist()))
    assert flat[float("inf")] == 255 and flat[float("-inf")] == 0 and flat[1.0] == 255 and flat[0.5] == 128 and flat[-1.0] == 0 and flat[2.0] == 255
    assert flat[float(np.nextafter(T(1), T(0)))] == 255 and flat[float(np.nextafter(T(1), T(2)))] == 255
    assert (got.reshape(-1)[30:36] == 0).all()                             # every NaN, whatever its sign, kind or payload


def test_the_tie_table_holds_real_ties_and_they_round_to_even(to_u8):
    vals, ks = PR.tie_table()
    assert vals.size == 1275 and (vals > 0).all() and (vals < 1).all()
    exact = vals * 255.0 == ks + 0.5
    assert (exact & (ks % 2 == 0)).sum() >= 64 and (exact & (ks % 2 == 1)).sum() >= 64         # (128 and 129 of the 1275)
    img = PR.as_frame(vals, np.float64, 17)
    assert img.shape == (25, 17, 3)
    got = PR.present(img).reshape(-1)
    assert np.array_equal(got, to_u8(img).reshape(-1))
    even = np.where(ks % 2 == 0, ks, ks + 1)
    assert np.array_equal(got[exact], even[exact])
    below, above = vals * 255.0 < ks + 0.5, vals * 255.0 > ks + 0.5
    assert np.array_equal(got[below], ks[below]) and np.array_equal(got[above], ks[above] + 1)
    # the same table in binary32: x * 255 in binary32 would land on k + 0.5 for many of these, binary64 does not
    img32 = PR.as_frame(vals, np.float32, 17)
    f32_ties = (img32.reshape(-1) * np.float32(255.0) == (ks + 0.5).astype(np.float32))
    f64_ties = img32.reshape(-1).astype(np.float64) * 255.0 == ks + 0.5
    assert f32_ties.sum() >= 64 and f64_ties.sum() <= 5
    assert np.array_equal(PR.present(img32), to_u8(img32))


def test_the_matrix():
    B = PR.bayer()
    assert sorted(B.reshape(-1).tolist()) == list(range(64))
    assert B[0].tolist() == [0, 32, 8, 40, 2, 34, 10, 42]
    t = PR.thresholds(8, 8)
    assert np.array_equal(t * 128, 2 * B + 1)                              # exact in binary64
    rng = np.random.default_rng(9)
    for y in list(rng.uniform(0, 255, 40)) + [0.0, 255.0, 127.5, 1.0 / 64, 254.99]:
        img = np.full((8, 8, 3), y / 255.0)
        got = PR.present(img, flags=PR.DITHER).astype(np.float64)
        yy = float(np.float64(y / 255.0) * 255.0)
        assert abs(got[:, :, 0].mean() - yy) <= 1.0 / 64 and np.array_equal(got[:, :, 0], got[:, :, 1]) and np.array_equal(got[:, :, 0], got[:, :, 2])
        assert got.max() - got.min() <= 1
    img = np.broadcast_to(np.array([0.3, 0.5, 0.7]), (24, 19, 3)).copy()                            # a constant colour, 24 x 19
    got = PR.present(img, flags=PR.DITHER)
    assert np.array_equal(got[8:, :], got[:-8, :]) and np.array_equal(got[:, 8:], got[:, :-8])       # periodic in 8 both ways
    assert np.unique(got[:, :, 0]).tolist() == [76, 77] and np.unique(got[:, :, 1]).tolist() == [127, 128]


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_flags_channels_and_nan_bytes(T):
    rng = np.random.default_rng(3)
    img = rng.uniform(-0.1, 1.1, (6, 9, 3)).astype(T)
    img[1, 2, 0] = np.nan                       # one channel only
    img[3, 4, :] = np.nan
    img[5, 8, 2] = np.nan
    base = PR.present(img)
    nb = PR.present(img, nan_rgb=(9, 8, 7))
    assert nb[1, 2].tolist() == [9] + base[1, 2, 1:].tolist() and nb[3, 4].tolist() == [9, 8, 7] and nb[5, 8].tolist() == base[5, 8, :2].tolist() + [7]
    keep = ~np.isnan(img)
    assert np.array_equal(nb[keep], base[keep])
    for flags in range(8):
        for ex in (1.0, 0.5, 3.0):
            a = PR.present(img, flags=flags & ~PR.BGR, exposure=ex, nan_rgb=(9, 8, 7))
            b = PR.present(img, flags=flags | PR.BGR, exposure=ex, nan_rgb=(9, 8, 7))
            assert np.array_equal(b, a[:, :, ::-1])                       # nan_rgb is swapped with the rest
            c = PR.present(img, channels=4, flags=flags, exposure=ex, nan_rgb=(9, 8, 7))
            assert c.shape == (6, 9, 4) and (c[:, :, 3] == 255).all()
            assert np.array_equal(c[:, :, :3], PR.present(img, flags=flags, exposure=ex, nan_rgb=(9, 8, 7)))
    lin = rng.uniform(0, 1, (4, 4, 3)).astype(T)
    assert np.array_equal(PR.present(lin, flags=PR.SQRT), PR.present(np.sqrt(lin.astype(np.float64))))
    assert np.array_equal(PR.present(lin, exposure=0.5), PR.present(lin.astype(np.float64) * 0.5))


def test_imageio_takes_uint8_frames_as_they_are(rtw, tmp_path):
    rng = np.random.default_rng(4)
    img = rng.uniform(0, 1, (5, 7, 3))
    u8 = PR.present(img)
    assert rtw.imageio.to_u8(u8) is u8
    p = rtw.imageio.save_ppm(u8, str(tmp_path / "a.ppm"))
    q = rtw.imageio.save_ppm(img, str(tmp_path / "b.ppm"))
    assert open(p, "rb").read() == open(q, "rb").read() and np.array_equal(rtw.imageio.load_ppm(p), u8)
    assert open(rtw.imageio.save_png(u8, str(tmp_path / "a.png")), "rb").read() == open(rtw.imageio.save_png(img, str(tmp_path / "b.png")), "rb").read()
    with pytest.raises(ValueError):
        rtw.imageio.save_ppm(PR.present(img, channels=4), str(tmp_path / "c.ppm"))
