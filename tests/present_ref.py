"""The numpy witness of the present stage: the definition of include/rtw_hip.h (rtw_present_*) restated step by step, in binary64, on
[H, W, 3] arrays.  It does not call imageio.to_u8: that the two agree with the defaults is what tests/test_present_ref.py checks.
Also the hand-made tables the CPU and the GPU tests share: special values and rounding ties."""
import numpy as np

DITHER, BGR, SQRT = 1, 2, 4          # RTW_PRESENT_*


def bayer():
    """B(r, c) = sum over b = 0..2 of (((r^c)>>b)&1) << (5-2b) | ((r>>b)&1) << (4-2b): the 8 x 8 Bayer index matrix"""
    B = np.zeros((8, 8), np.int64)
    for r in range(8):
        for c in range(8):
            B[r, c] = sum(((((r ^ c) >> b) & 1) << (5 - 2 * b)) | (((r >> b) & 1) << (4 - 2 * b)) for b in range(3))
    return B


def thresholds(H, W):
    """t of every pixel: (B(i mod 8, j mod 8) + 0.5) / 64, exact in binary64"""
    B = bayer()
    i, j = np.arange(H) % 8, np.arange(W) % 8
    return (B[i][:, j].astype(np.float64) + 0.5) / 64.0


def present(image, channels=3, flags=0, exposure=1.0, nan_rgb=(0, 0, 0)):
    """``image`` [H, W, 3] of float32 or float64 -> uint8 [H, W, channels], row-major"""
    x = np.asarray(image)
    assert x.ndim == 3 and x.shape[2] == 3 and x.dtype in (np.float32, np.float64) and channels in (3, 4)
    H, W = x.shape[:2]
    with np.errstate(invalid="ignore"):                              # (a signalling NaN raises the flag when it is widened)
        v = x.astype(np.float64)                                     # 1. exact
    nan = np.isnan(v)                                                # 2. per channel
    v = np.where(nan, 0.0, v)
    with np.errstate(over="ignore"):
        v = v * np.float64(exposure)                                 # 3.
    v = np.minimum(np.maximum(v, 0.0), 1.0)                          # 4.
    if flags & SQRT:
        v = np.sqrt(v)                                               # 5. (IEEE: correctly rounded)
    y = v * 255.0                                                    # 6.
    if flags & DITHER:
        q = np.minimum(np.floor(y + thresholds(H, W)[:, :, None]), 255.0)
    else:
        q = np.rint(y)                                               # 7. ties to even
    out = np.full((H, W, channels), 255, np.uint8)
    rgb = q.astype(np.uint8)
    for k in range(3):
        rgb[:, :, k][nan[:, :, k]] = nan_rgb[k]
    out[:, :, :3] = rgb[:, :, ::-1] if flags & BGR else rgb
    return out


def special_values(T):
    """+-0, denormals, +-inf, quiet and signalling NaNs with payloads and either sign, values below 0 and above 1, 1 and its neighbours"""
    T = np.dtype(T).type
    fi = np.finfo(T)
    vals = [0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny / 2, -fi.tiny / 2, fi.tiny, np.inf, -np.inf,
            -1.0, -1e-30, -0.5, -fi.max, 1.5, 2.0, 255.0, 1e30, fi.max, 1.0, np.nextafter(T(1), T(0)), np.nextafter(T(1), T(2)),
            0.5, 0.25, 0.75, 1.0 / 3.0, 1.0 / 255.0, 0.5 / 255.0, 254.5 / 255.0, 0.1, 0.9]
    a = np.array(vals, dtype=T)
    if T is np.float32:
        nans = np.array([0x7fc00000, 0xffc00000, 0x7fc12345, 0x7fa00001, 0xff800001, 0x7fffffff], np.uint32).view(np.float32)
    else:
        nans = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000012345678, 0x7ff4000000000001, 0xfff0000000000001,
                         0x7fffffffffffffff], np.uint64).view(np.float64)
    assert np.isnan(nans).all()
    return np.concatenate([a, nans])


def tie_table():
    """For k = 0..254 the double nearest (k + 0.5) / 255 and its neighbours at +-1 and +-2 ulps: 1275 values in (0, 1), many of which
    have v * 255.0 == k + 0.5 exactly in binary64 -> (values float64 [1275], k int64 [1275])"""
    vals, ks = [], []
    for k in range(255):
        c = np.float64(k + 0.5) / np.float64(255.0)
        lo1 = np.nextafter(c, -np.inf)
        hi1 = np.nextafter(c, np.inf)
        vals += [np.nextafter(lo1, -np.inf), lo1, c, hi1, np.nextafter(hi1, np.inf)]
        ks += [k] * 5
    return np.array(vals, np.float64), np.array(ks, np.int64)


def as_frame(values, T, W):
    """a table laid out as a frame [H, W, 3] of T, row-major over (i, j, k), padded with 0.25"""
    values = np.asarray(values)
    n = -(-values.size // (3 * W)) * 3 * W
    a = np.full(n, 0.25, dtype=T)
    a[:values.size] = values.astype(T)
    return a.reshape(-1, W, 3)
