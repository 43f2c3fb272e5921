"""The witness of the feature-guided upsampler (include/rtw_hip.h rtw_upsample_*): the definition restated in numpy from nothing of the
product.  The small frame is prepared and filtered by the denoiser's witness (denoise_ref.prepare / denoise_ref.level); everything at the
full size is restated here.  Every intermediate has the element type T (asserted); numpy rounds every operation once and never fuses.

    upsample(image_lo, feat_lo, feat_hi, T, ...)          vectorised: whole full-size frames per tap
    upsample_scalar(image_lo, feat_lo, feat_hi, T, ...)   the same definition one full-size pixel and one numpy scalar at a time
    coords(small, full, T)                                one axis of the position in the small frame: x0, r_x, fx
    handmade_pair(h, w, H, W, T, seed)                    a small and a full frame drawn independently, so that the guides disagree
    census(...)                                           which branches of the definition a pair reaches, counted on the witness alone
Arrays are indexed [i, j, channel] (row, column): the library's memory is the transpose, pixel (i, j) at j*rows + i."""
import numpy as np

import denoise_ref as DR

DEFAULTS = dict(levels=2, m=1, sigma_color=0.5, sigma_depth=0.1, sigma_albedo=0.2, demodulate=True, gamma=1)
_is = DR._is

#: the frames of tests/test_gpu_upsample.py, small (w, h) -> full (W, H), and the committed seeds of their hand-made pairs
PAIRS = [((1, 1), (1, 1)), ((1, 1), (4, 3)), ((5, 3), (10, 6)), ((5, 3), (11, 7)), ((18, 10), (37, 23)), ((35, 20), (70, 41)), ((70, 41), (70, 41)),
         ((9, 40), (10, 300))]
SEEDS = {np.float32: 21, np.float64: 22}


def coords(small, full, T):
    """-> x0 [full] int64, r_x [full] int64 in [0, 2*full), fx [full] of type T: exact integers, then two conversions and one quotient"""
    T = np.dtype(T).type
    c = np.arange(full, dtype=np.int64)
    num = (2 * c + 3) * small - 3 * full
    x0 = num // (2 * full)                                  # floor, also of negative numerators
    r = num - x0 * (2 * full)
    assert ((r >= 0) & (r < 2 * full)).all()
    f = r.astype(T) / T(2 * full)
    _is(T, f)
    return x0, r, f


def tent(o, f, T):
    """the spatial weight of one axis at tap offset o: 1 - |o - f| / 2"""
    T = np.dtype(T).type
    k = T(1) - np.abs(T(o) - f) * T(0.5)
    _is(T, np.asarray(k))
    return k


def tap_constants(sigma_albedo, sigma_depth, T):
    """what the host computes in binary64 -> (inv_sa, inv_sz) of type T"""
    T = np.dtype(T).type
    with np.errstate(all="ignore"):
        return (T(np.float64(1.0) / np.float64(float(sigma_albedo) * float(sigma_albedo))),
                T(np.float64(1.0) / np.float64(float(sigma_depth) * float(sigma_depth))))


def small_frame(image_lo, feat_lo, T, levels, m, sigma_color, sigma_depth, demodulate):
    """the small frame as the taps read it -> valid, has, e (after `levels` passes, none of them final), n, z, cov, a"""
    valid, has, e, n, z, cov, a = DR.prepare(image_lo, feat_lo, T, demodulate)
    for k in range(levels):
        e = DR.level(e, valid, has, n, z, cov, k, m, sigma_color, sigma_depth, T)
    return valid, has, e, n, z, cov, a


def full_guides(feat_hi, T, demodulate):
    """-> valid, has [H, W] bool; n [H, W, 3], z, cov [H, W], a [H, W, 3] of type T"""
    T = np.dtype(T).type
    F = np.asarray(feat_hi)
    _is(T, F)
    with np.errstate(all="ignore"):
        valid = np.isfinite(F).all(axis=2)
        cov = F[..., 7]
        has = valid & (cov > T(0))
        dv = np.where(has, cov, T(1))
        n = np.where(has[..., None], F[..., 3:6] / dv[..., None], T(0))
        z = np.where(has, F[..., 6] / dv, T(0))
        a = np.maximum(F[..., 0:3], T(2.0 ** -6)) if demodulate else np.ones(F.shape[:2] + (3,), T)
    _is(T, dv, n, z, a, cov)
    return valid, has, n, z, cov, a


def upsample(image_lo, feat_lo, feat_hi, T, levels=2, m=1, sigma_color=0.5, sigma_depth=0.1, sigma_albedo=0.2, demodulate=True, gamma=1, details=None):
    """the definition, vectorised -> out [H, W, 3] of type T; NaN where the pixel is not valid.  `details`: a dict that receives the sums"""
    T = np.dtype(T).type
    valid, has, e, n, z, cov, a = small_frame(image_lo, feat_lo, T, levels, m, sigma_color, sigma_depth, demodulate)
    h, w = valid.shape
    validP, hasP, nP, zP, covP, aP = full_guides(feat_hi, T, demodulate)
    H, W = validP.shape
    assert 1 <= w <= W and 1 <= h <= H
    inv_sa, inv_sz = tap_constants(sigma_albedo, sigma_depth, T)
    x0, _, fx = coords(w, W, T)
    y0, _, fy = coords(h, H, T)
    sum_w, sum_s = np.zeros((H, W), T), np.zeros((H, W), T)
    sum_e, sum_se = np.zeros((H, W, 3), T), np.zeros((H, W, 3), T)
    outside = 0
    with np.errstate(all="ignore"):
        for b in range(-1, 3):
            kx = tent(b, fx, T)
            for c in range(-1, 3):
                ky = tent(c, fy, T)
                s = ky[:, None] * kx[None, :]
                qi, qj = y0 + c, x0 + b
                inside = ((qi >= 0) & (qi < h))[:, None] & ((qj >= 0) & (qj < w))[None, :]
                outside += int((~inside).sum())
                gi, gj = np.clip(qi, 0, h - 1)[:, None], np.clip(qj, 0, w - 1)[None, :]
                ok = inside & valid[gi, gj]
                eq, nq, zq, cq, hq, aq = e[gi, gj], n[gi, gj], z[gi, gj], cov[gi, gj], has[gi, gj], a[gi, gj]
                da = aP - aq
                dA = (da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]
                w_a = T(1) / (T(1) + dA * inv_sa)
                t_v = T(1) - np.abs(covP - cq)
                w_v = np.where(t_v > T(0), t_v, T(0))
                wt = (s * w_a) * w_v
                dot = (nP[..., 0] * nq[..., 0] + nP[..., 1] * nq[..., 1]) + nP[..., 2] * nq[..., 2]
                t = np.where(dot > T(0), dot, T(0))
                for _ in range(m):
                    t = t * t
                zs = zP + zq
                r = (zP - zq) / np.where(zs > T(0), zs, T(1))
                w_z = T(1) / (T(1) + (r * r) * inv_sz)
                wg = (wt * t) * w_z
                _is(T, s, da, dA, w_a, t_v, w_v, wt, dot, t, zs, r, w_z, wg)
                wt = np.where(hasP & hq, wg, wt)
                term, sterm = wt[..., None] * eq, s[..., None] * eq
                _is(T, wt, term, sterm)
                # a skipped tap adds nothing: the sums are never -0 (they start at +0), so adding +0 is skipping
                sum_w = sum_w + np.where(ok, wt, T(0))
                sum_e = sum_e + np.where(ok[..., None], term, T(0))
                sum_s = sum_s + np.where(ok, s, T(0))
                sum_se = sum_se + np.where(ok[..., None], sterm, T(0))
                _is(T, sum_w, sum_e, sum_s, sum_se)
        guided = sum_w > T(0)
        den = np.where(guided, sum_w, sum_s)
        eo = np.where(guided[..., None], sum_e, sum_se) / den[..., None]
        good = validP & (den > T(0))
        out = eo * aP if demodulate else eo.copy()
        if gamma:
            out = np.sqrt(out)
    _is(T, den, eo, out)
    out[~good] = np.nan
    if details is not None:
        details.update(sum_w=sum_w, sum_s=sum_s, guided=guided, validP=validP, good=good, outside=outside, e=e, a=a, valid=valid)
    return out


def upsample_scalar(image_lo, feat_lo, feat_hi, T, levels=2, m=1, sigma_color=0.5, sigma_depth=0.1, sigma_albedo=0.2, demodulate=True, gamma=1):
    """the definition, one full-size pixel at a time on numpy scalars of type T (for tiny frames)"""
    T = np.dtype(T).type
    valid, has, e, n, z, cov, a = small_frame(image_lo, feat_lo, T, levels, m, sigma_color, sigma_depth, demodulate)
    h, w = valid.shape
    F = np.asarray(feat_hi)
    _is(T, F)
    H, W = F.shape[:2]
    assert 1 <= w <= W and 1 <= h <= H
    inv_sa, inv_sz = tap_constants(sigma_albedo, sigma_depth, T)
    one, zero, half, floor_ = T(1), T(0), T(0.5), T(2.0 ** -6)
    out = np.full((H, W, 3), np.nan, T)
    with np.errstate(all="ignore"):
        for i in range(H):
            for j in range(W):
                f = F[i, j]
                if not bool(np.isfinite(f).all()):
                    continue
                covP = f[7]
                hasP = bool(covP > zero)
                nP = (f[3] / covP, f[4] / covP, f[5] / covP) if hasP else (zero, zero, zero)
                zP = f[6] / covP if hasP else zero
                aP = tuple(max(f[k], floor_) for k in range(3)) if demodulate else (one, one, one)
                num_x, num_y = (2 * j + 3) * w - 3 * W, (2 * i + 3) * h - 3 * H            # Python integers: exact
                x0, y0 = num_x // (2 * W), num_y // (2 * H)
                # (through np.int64: one conversion, rounded once)
                fx, fy = np.int64(num_x - x0 * 2 * W).astype(T) / T(2 * W), np.int64(num_y - y0 * 2 * H).astype(T) / T(2 * H)
                sw, ss, se, sse = zero, zero, [zero] * 3, [zero] * 3
                for b in range(-1, 3):
                    kx = one - abs(T(b) - fx) * half
                    for c in range(-1, 3):
                        ky = one - abs(T(c) - fy) * half
                        s = ky * kx
                        qi, qj = y0 + c, x0 + b
                        if not (0 <= qi < h and 0 <= qj < w) or not valid[qi, qj]:
                            continue
                        eq, aq = e[qi, qj], a[qi, qj]
                        d0, d1, d2 = aP[0] - aq[0], aP[1] - aq[1], aP[2] - aq[2]
                        dA = (d0 * d0 + d1 * d1) + d2 * d2
                        w_a = one / (one + dA * inv_sa)
                        t_v = one - abs(covP - cov[qi, qj])
                        w_v = t_v if t_v > zero else zero
                        wt = (s * w_a) * w_v
                        if hasP and has[qi, qj]:
                            nq, zq = n[qi, qj], z[qi, qj]
                            dot = (nP[0] * nq[0] + nP[1] * nq[1]) + nP[2] * nq[2]
                            t = dot if dot > zero else zero
                            for _ in range(m):
                                t = t * t
                            zs = zP + zq
                            r = (zP - zq) / (zs if zs > zero else one)
                            w_z = one / (one + (r * r) * inv_sz)
                            wt = (wt * t) * w_z
                        assert type(wt) is T and type(s) is T and type(fx) is T
                        sw, ss = sw + wt, ss + s
                        for k in range(3):
                            se[k] = se[k] + wt * eq[k]
                            sse[k] = sse[k] + s * eq[k]
                if sw > zero:
                    eo = [se[k] / sw for k in range(3)]
                elif ss > zero:
                    eo = [sse[k] / ss for k in range(3)]
                else:
                    continue
                for k in range(3):
                    v = eo[k] * aP[k] if demodulate else eo[k]
                    assert type(v) is T
                    out[i, j, k] = np.sqrt(v) if gamma else v
    return out


BLOCK = 5            # the side of a planted block of small pixels: a 4 x 4 tap footprint fits inside it


def _blocks(h, w):
    """the three planted blocks of the small frame, (row, column) of their first pixel, along the longer axis; none in a frame too small"""
    if min(h, w) < BLOCK or max(h, w) < 3 * BLOCK + 3:
        return []
    if w >= h:
        return [((h - BLOCK) // 2, 1 + 6 * k) for k in range(3)]
    return [(1 + 6 * k, (w - BLOCK) // 2) for k in range(3)]


def _inside_block(small, full, first):
    """the full-size indices of one axis whose four taps all lie in [first, first + BLOCK)"""
    x0 = coords(small, full, np.float64)[0]
    return np.nonzero((x0 - 1 >= first) & (x0 + 2 <= first + BLOCK - 1))[0]


def handmade_pair(h, w, H, W, T, seed):
    """A small and a full frame -> (image_lo [h, w, 3], feat_lo [h, w, 8], feat_hi [H, W, 8]) of type T, drawn INDEPENDENTLY with
    denoise_ref.handmade's regimes (coverage 0 / fractional / 1, tiny albedo, z <= 0, pixels that are not finite), so that the guides of a
    full-size pixel and of its taps disagree in every way.  Small frames of 18 pixels or more on their longer side and 5 on the shorter
    also carry three planted 5 x 5 blocks, so that every branch of the end step is reached (census):
        block 0   not valid (a NaN image): the full-size pixels whose taps all lie inside have no valid tap
        block 1   normal (1, 0, 0) under full-size normals (0, 1, 0): every guided weight is exactly 0, the spatial fallback decides
        block 2   normal (1, 0, 0) under full-size normals at a dot product of 2^-1.1 (binary32) / 2^-8.2 (binary64): with m = 7 the
                  normal weight dot^128 -- and with it sum_w -- is a subnormal number"""
    T = np.dtype(T).type
    image_lo, feat_lo = DR.handmade(h, w, T, seed)
    feat_hi = DR.handmade(H, W, T, seed + 1000)[1]
    d = 2.0 ** (-1.1 if T is np.float32 else -8.2)
    for k, (r0, c0) in enumerate(_blocks(h, w)):
        rows, cols = _inside_block(h, H, r0), _inside_block(w, W, c0)
        assert len(rows) and len(cols)
        lo = np.s_[r0:r0 + BLOCK, c0:c0 + BLOCK]
        image_lo[lo] = (np.arange(BLOCK * BLOCK * 3).reshape(BLOCK, BLOCK, 3) % 7 + 1) / 8.0
        feat_lo[lo] = np.array([0.5, 0.25, 0.75, 1.0, 0.0, 0.0, 5.0, 1.0], T)
        if k == 0:
            image_lo[lo] = np.nan
        normal = [0.0, 1.0, 0.0] if k <= 1 else [d, np.sqrt(1.0 - d * d), 0.0]
        feat_hi[np.ix_(rows, cols)] = np.array([0.5, 0.25, 0.75] + normal + [5.0, 1.0]).astype(T)
    return image_lo, feat_lo, feat_hi


def census(image_lo, feat_lo, feat_hi, T, **params):
    """which branches of the definition the pair reaches, counted on the witness alone: full-size pixels decided by the spatial fallback, NaN
    because no tap is valid, NaN because valid(P) is false, with a subnormal sum_w, and the taps skipped as outside the small frame"""
    T = np.dtype(T).type
    d = {}
    upsample(image_lo, feat_lo, feat_hi, T, details=d, **params)
    tiny = np.finfo(T).tiny
    with np.errstate(all="ignore"):
        return dict(fallback=int((d["validP"] & ~d["guided"] & (d["sum_s"] > 0)).sum()),
                    no_valid_tap=int((d["validP"] & ~d["good"]).sum()),
                    not_valid_P=int((~d["validP"]).sum()),
                    subnormal_sum_w=int((d["validP"] & (d["sum_w"] > 0) & (d["sum_w"] < tiny)).sum()),
                    taps_outside=d["outside"])


def box_half(a):
    """[2h, 2w, c] -> [h, w, c]: the mean of every 2 x 2 block, in the array's own type ((p + q) + (r + s)) * 0.25"""
    return ((a[0::2, 0::2] + a[1::2, 0::2]) + (a[0::2, 1::2] + a[1::2, 1::2])) * a.dtype.type(0.25)


bits, same_bits = DR.bits, DR.same_bits
