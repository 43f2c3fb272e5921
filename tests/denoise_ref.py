"""The witness of the feature-guided denoiser (include/rtw_hip.h rtw_denoise_*): the definition restated in numpy from nothing of the
product.  Every intermediate has the element type T (asserted); numpy rounds every operation once and never fuses.

    denoise(image, features, T, ...)          vectorised: whole frames per tap
    denoise_scalar(image, features, T, ...)   the same definition one pixel and one numpy scalar at a time, for tiny frames
    handmade(H, W, T, seed)                   a hand-made frame with every regime of the definition; census(...) counts them
    step_frame(T, seed)                       a vertical step in albedo and normal under noise
Arrays are indexed [i, j, channel] (row, column): the library's memory is the transpose, pixel (i, j) at j*H + i."""
import numpy as np

K = (0.375, 0.25, 0.0625)
DEFAULTS = dict(levels=3, m=1, sigma_color=0.5, sigma_depth=0.1, demodulate=True, gamma=1)


def _is(T, *arrs):
    for a in arrs:
        assert a.dtype == np.dtype(T), (a.dtype, T)


def level_constants(k, sigma_color, sigma_depth, T):
    """what the host computes in binary64 for level k -> (inv_sc, inv_sz) of type T"""
    sc = float(sigma_color) * 2.0 ** -k
    with np.errstate(all="ignore"):
        return T(np.float64(1.0) / np.float64(sc * sc)), T(np.float64(1.0) / np.float64(float(sigma_depth) * float(sigma_depth)))


def prepare(image, features, T, demodulate):
    """-> valid, has [H, W] bool; e [H, W, 3], n [H, W, 3], z, cov [H, W], a [H, W, 3] of type T"""
    T = np.dtype(T).type
    c, f = np.asarray(image), np.asarray(features)
    _is(T, c, f)
    with np.errstate(all="ignore"):
        valid = np.isfinite(c).all(axis=2) & np.isfinite(f).all(axis=2)
        cov = f[..., 7]
        has = valid & (cov > T(0))
        dv = np.where(has, cov, T(1))
        n = np.where(has[..., None], f[..., 3:6] / dv[..., None], T(0))
        z = np.where(has, f[..., 6] / dv, T(0))
        if demodulate:
            a = np.maximum(f[..., 0:3], T(2.0 ** -6))
            e = c / a
        else:
            a = np.ones_like(c)
            e = c.copy()
    _is(T, dv, n, z, a, e, cov)
    return valid, has, e, n, z, cov, a


def _shift(arr, oi, oj, fill):
    """out[i, j] = arr[i + oi, j + oj] inside the frame, `fill` outside"""
    H, W = arr.shape[:2]
    out = np.full_like(arr, fill)
    i0, i1 = max(0, -oi), min(H, H - oi)
    j0, j1 = max(0, -oj), min(W, W - oj)
    if i0 < i1 and j0 < j1:
        out[i0:i1, j0:j1] = arr[i0 + oi:i1 + oi, j0 + oj:j1 + oj]
    return out


def level(e, valid, has, n, z, cov, k, m, sigma_color, sigma_depth, T):
    """one a-trous pass with step 2^k over the whole frame -> e' (pixels that are not valid hold garbage)"""
    T = np.dtype(T).type
    s = 1 << k
    inv_sc, inv_sz = level_constants(k, sigma_color, sigma_depth, T)
    H, W = valid.shape
    sum_w = np.zeros((H, W), T)
    sum_e = np.zeros((H, W, 3), T)
    with np.errstate(all="ignore"):
        for dj in range(-2, 3):
            for di in range(-2, 3):
                h = T(K[abs(di)] * K[abs(dj)])
                if di == 0 and dj == 0:
                    sum_w = sum_w + h
                    sum_e = sum_e + h * e
                    _is(T, sum_w, sum_e)
                    continue
                ok = _shift(valid, s * di, s * dj, False)                 # inside the frame and valid
                eq = _shift(e, s * di, s * dj, T(0))
                nq = _shift(n, s * di, s * dj, T(0))
                zq = _shift(z, s * di, s * dj, T(0))
                cq = _shift(cov, s * di, s * dj, T(0))
                hq = _shift(has, s * di, s * dj, False)
                d = e - eq
                dc = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                w_c = T(1) / (T(1) + dc * inv_sc)
                t_v = T(1) - np.abs(cov - cq)
                w_v = np.where(t_v > T(0), t_v, T(0))
                w = (h * w_c) * w_v
                dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                t = np.where(dot > T(0), dot, T(0))
                for _ in range(m):
                    t = t * t
                zs = z + zq
                r = (z - zq) / np.where(zs > T(0), zs, T(1))
                w_z = T(1) / (T(1) + (r * r) * inv_sz)
                wg = (w * t) * w_z
                _is(T, d, dc, w_c, t_v, w_v, w, dot, t, zs, r, w_z, wg)
                w = np.where(has & hq, wg, w)
                term = w[..., None] * eq
                _is(T, w, term)
                # a skipped tap adds nothing: the sums are never -0 (they start at +0), so adding +0 is skipping
                sum_w = sum_w + np.where(ok, w, T(0))
                sum_e = sum_e + np.where(ok[..., None], term, T(0))
                _is(T, sum_w, sum_e)
        out = sum_e / sum_w[..., None]
    _is(T, out)
    return out


def finish(e, a, valid, demodulate, gamma, T):
    T = np.dtype(T).type
    with np.errstate(all="ignore"):
        out = e * a if demodulate else e.copy()
        if gamma:
            out = np.sqrt(out)
    _is(T, out)
    out[~valid] = np.nan
    return out


def denoise(image, features, T, levels=3, m=1, sigma_color=0.5, sigma_depth=0.1, demodulate=True, gamma=1):
    """the definition, vectorised -> out [H, W, 3] of type T; NaN where the pixel is not valid"""
    valid, has, e, n, z, cov, a = prepare(image, features, T, demodulate)
    for k in range(levels):
        e = level(e, valid, has, n, z, cov, k, m, sigma_color, sigma_depth, T)
    return finish(e, a, valid, demodulate, gamma, T)


def denoise_scalar(image, features, T, levels=3, m=1, sigma_color=0.5, sigma_depth=0.1, demodulate=True, gamma=1):
    """the definition, one pixel at a time on numpy scalars of type T (for tiny frames)"""
    T = np.dtype(T).type
    c, f = np.asarray(image), np.asarray(features)
    _is(T, c, f)
    H, W = c.shape[:2]
    one, zero = T(1), T(0)
    valid = [[bool(np.isfinite(c[i, j]).all() and np.isfinite(f[i, j]).all()) for j in range(W)] for i in range(H)]
    has = [[valid[i][j] and bool(f[i, j, 7] > zero) for j in range(W)] for i in range(H)]
    n = [[None] * W for _ in range(H)]
    z = [[zero] * W for _ in range(H)]
    a = [[None] * W for _ in range(H)]
    e = [[None] * W for _ in range(H)]
    with np.errstate(all="ignore"):
        for i in range(H):
            for j in range(W):
                cv = f[i, j, 7]
                if has[i][j]:
                    n[i][j] = (f[i, j, 3] / cv, f[i, j, 4] / cv, f[i, j, 5] / cv)
                    z[i][j] = f[i, j, 6] / cv
                else:
                    n[i][j] = (zero, zero, zero)
                if demodulate:
                    a[i][j] = tuple(max(f[i, j, k], T(2.0 ** -6)) if valid[i][j] else one for k in range(3))
                    e[i][j] = tuple(c[i, j, k] / a[i][j][k] for k in range(3))
                else:
                    a[i][j] = (one, one, one)
                    e[i][j] = tuple(c[i, j, k] for k in range(3))
        for lv in range(levels):
            s = 1 << lv
            inv_sc, inv_sz = level_constants(lv, sigma_color, sigma_depth, T)
            nxt = [[None] * W for _ in range(H)]
            for i in range(H):
                for j in range(W):
                    if not valid[i][j]:
                        nxt[i][j] = e[i][j]
                        continue
                    ep, np_, zp, cp = e[i][j], n[i][j], z[i][j], f[i, j, 7]
                    sw, se = zero, [zero, zero, zero]
                    for dj in range(-2, 3):
                        for di in range(-2, 3):
                            h = T(K[abs(di)] * K[abs(dj)])
                            if di == 0 and dj == 0:
                                w, eq = h, ep
                            else:
                                qi, qj = i + s * di, j + s * dj
                                if not (0 <= qi < H and 0 <= qj < W) or not valid[qi][qj]:
                                    continue
                                eq, nq, zq, cq = e[qi][qj], n[qi][qj], z[qi][qj], f[qi, qj, 7]
                                d0, d1, d2 = ep[0] - eq[0], ep[1] - eq[1], ep[2] - eq[2]
                                dc = (d0 * d0 + d1 * d1) + d2 * d2
                                w_c = one / (one + dc * inv_sc)
                                t_v = one - abs(cp - cq)
                                w_v = t_v if t_v > zero else zero
                                w = (h * w_c) * w_v
                                if has[i][j] and has[qi][qj]:
                                    dot = (np_[0] * nq[0] + np_[1] * nq[1]) + np_[2] * nq[2]
                                    t = dot if dot > zero else zero
                                    for _ in range(m):
                                        t = t * t
                                    zs = zp + zq
                                    r = (zp - zq) / (zs if zs > zero else one)
                                    w_z = one / (one + (r * r) * inv_sz)
                                    w = (w * t) * w_z
                            assert type(w) is T
                            sw = sw + w
                            for k in range(3):
                                se[k] = se[k] + w * eq[k]
                    nxt[i][j] = tuple(se[k] / sw for k in range(3))
                    assert all(type(x) is T for x in nxt[i][j]) and type(sw) is T
            e = nxt
        out = np.full((H, W, 3), np.nan, T)
        for i in range(H):
            for j in range(W):
                if not valid[i][j]:
                    continue
                for k in range(3):
                    v = e[i][j][k] * a[i][j][k] if demodulate else e[i][j][k]
                    out[i, j, k] = np.sqrt(v) if gamma else v
    return out


def handmade(H, W, T, seed):
    """A hand-made frame -> (image [H, W, 3], features [H, W, 8]) of type T: coverage 0, fractional and 1; albedo channels below 2^-6;
    depths z <= 0 under a positive coverage; and, in frames of 12 pixels or more, three or more pixels that are not finite -- a NaN in
    the image, an inf in the coverage, a -inf in a normal --, the first of them on the border."""
    T = np.dtype(T).type
    rng = np.random.default_rng(seed)
    cov = rng.choice([0.0, 1.0, -1.0], size=(H, W), p=[0.25, 0.4, 0.35])
    frac = rng.integers(1, 8, size=(H, W)) / 8.0
    cov = np.where(cov < 0, frac, cov)
    albedo = rng.uniform(0.05, 1.0, size=(H, W, 3))
    albedo = np.where(rng.random((H, W, 3)) < 0.15, albedo * 2.0 ** -8, albedo)
    v = rng.normal(size=(H, W, 3))
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    v = np.where(rng.random((H, W, 1)) < 0.5, np.array([0.0, 0.6, 0.8]), v)            # half of the pixels share a plane
    normal = v * cov[..., None]
    z = rng.uniform(1.0, 20.0, size=(H, W))
    z = np.where(rng.random((H, W)) < 0.12, -z * (rng.random((H, W)) < 0.5), z)        # z <= 0: negative or exactly 0
    depth = z * cov
    image = albedo * rng.uniform(0.0, 2.0, size=(H, W, 1)) * rng.uniform(0.5, 1.5, size=(H, W, 3))
    feat = np.concatenate([albedo, normal, depth[..., None], cov[..., None]], axis=2)
    image, feat = image.astype(T), feat.astype(T)
    if H * W >= 12:
        border = [(i, j) for i in range(H) for j in range(W) if i in (0, H - 1) or j in (0, W - 1)]
        bad = [border[int(rng.integers(len(border)))]]
        while len(bad) < 4:
            pq = (int(rng.integers(H)), int(rng.integers(W)))
            if pq not in bad:
                bad.append(pq)
        image[bad[0] + (1,)] = np.nan
        feat[bad[1] + (7,)] = np.inf
        feat[bad[2] + (4,)] = -np.inf
        image[bad[3] + (0,)] = np.inf
    return image, feat


def census(image, feat):
    """what a hand-made frame holds, counted on its valid pixels (non-finite ones: on all)"""
    valid = np.isfinite(image).all(axis=2) & np.isfinite(feat).all(axis=2)
    H, W = valid.shape
    cov = feat[..., 7]
    edge = np.zeros((H, W), bool)
    edge[[0, -1], :] = True
    edge[:, [0, -1]] = True
    with np.errstate(all="ignore"):
        has = valid & (cov > 0)
        return dict(cov0=int((valid & (cov == 0)).sum()), cov_frac=int((valid & (cov > 0) & (cov < 1)).sum()), cov1=int((valid & (cov == 1)).sum()),
                    tiny_albedo=int((valid[..., None] & (feat[..., 0:3] < 2.0 ** -6)).sum()), z_le_0=int((has & (feat[..., 6] <= 0)).sum()),
                    non_finite=int((~valid).sum()), non_finite_border=int((~valid & edge).sum()))


def step_frame(T, seed, H=16, W=24, noise=0.3):
    """A vertical step at column W/2 in albedo and normal (orthogonal normals, one depth, full coverage) under multiplicative noise
    -> (noisy image, clean image, features)"""
    T = np.dtype(T).type
    rng = np.random.default_rng(seed)
    left = np.arange(W) < W // 2
    albedo = np.where(left[None, :, None], np.array([0.8, 0.25, 0.2]), np.array([0.2, 0.3, 0.85])) * np.ones((H, 1, 1))
    normal = np.where(left[None, :, None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0])) * np.ones((H, 1, 1))
    feat = np.concatenate([albedo, normal, np.full((H, W, 1), 5.0), np.ones((H, W, 1))], axis=2).astype(T)
    clean = albedo.astype(T)
    noisy = (albedo * (1.0 + rng.uniform(-noise, noise, size=(H, W, 3)))).astype(T)
    return noisy, clean, feat


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(got, ref):
    """NaN pixels as a set, everything else on the bits"""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    gn, rn = np.isnan(got), np.isnan(ref)
    return bool(np.array_equal(gn, rn) and np.array_equal(bits(got)[~gn], bits(ref)[~rn]))
