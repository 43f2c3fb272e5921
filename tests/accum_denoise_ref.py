"""The witness of the accumulator side of the denoiser (include/rtw_hip.h rtw_accum_features_*, rtw_accum_noise_*,
rtw_guided_filter_device_*, rtw_accum_filtered_*): the definitions restated from nothing of the product.  A helper module, not a test.

    noise_map(words, chunks, ...)              the per-pixel noise map from accumulator words and C_t: Python integers and binary64
    guided(image, features, noise, T, ...)     the noise-guided filter, vectorised numpy with asserted dtypes
    guided_scalar(...)                         the same definition one pixel and one numpy scalar at a time
    tile_prefix_features(it, T, chunks, ...)   tile t's features over the chunks [0, C_t), assembled from features_ref
    adaptive_words(...)                        an adaptive accumulator from oracle samples: words and C_t by the written rule
tests/denoise_ref.py is reused by import, unchanged: prepare, the shifts, the level constants and the end step are the plain filter's.
Arrays are indexed [i, j, ...] (row, column); the library keeps pixel (i, j) at j*H + i."""
import math

import numpy as np

import accum_words as AW
import denoise_ref as DR
import features_ref as FR

V_MIN, V_MAX = 2.0 ** -40, 2.0 ** 40
GUIDED_DEFAULTS = dict(levels=3, m=1, sigma_color=1.0, sigma_depth=0.1, demodulate=True, gamma=1)


# ---- the noise map ---------------------------------------------------------------------------------------------------------------------
def pixel_rho(w, n, floor):
    """rho of one pixel from its 8 words and the samples n its tile holds; None: the pixel is poisoned"""
    if int(w[6]) != 0:
        return None
    D = float(abs(AW.signed64(w[7]))) * 2.0 ** -24
    y = (AW.sum_to_double(AW.signed128(w[0], w[1])) + AW.sum_to_double(AW.signed128(w[2], w[3]))) + AW.sum_to_double(AW.signed128(w[4], w[5]))
    M = max(max(y, 0.0), float(floor) * float(n))
    return D / M if M > 0.0 else 0.0


def noise_map(words, chunks, width, height, spp, chunk_spp, floor, T, radius=1):
    """-> [H, W] of dtype T: the binomial mean of rho over the (2 radius + 1)^2 neighbours inside the frame that are not poisoned
    (radius 1: the definition; 2: the 5 x 5 variant of the sweep), NaN where the pixel itself is poisoned.  ``chunks``: C_t in tile
    order t = tj * tiles_i + ti."""
    T = np.dtype(T).type
    H, W = int(height), int(width)
    words = np.asarray(words)
    assert words.shape == (H, W, 8)
    tiles_i = (H + 7) // 8
    rho = [[None] * W for _ in range(H)]
    for i in range(H):
        for j in range(W):
            n = min(int(spp), int(chunks[(j // 8) * tiles_i + i // 8]) * int(chunk_spp))
            rho[i][j] = pixel_rho(words[i, j], n, floor)
    k1 = {1: (1.0, 2.0, 1.0), 2: (1.0, 4.0, 6.0, 4.0, 1.0)}[radius]
    out = np.full((H, W), np.nan, T)
    for i in range(H):
        for j in range(W):
            if rho[i][j] is None:
                continue
            num = den = 0.0
            for dj in range(-radius, radius + 1):
                for di in range(-radius, radius + 1):
                    qi, qj = i + di, j + dj
                    if not (0 <= qi < H and 0 <= qj < W) or rho[qi][qj] is None:
                        continue
                    b = k1[di + radius] * k1[dj + radius]
                    num = num + b * rho[qi][qj]
                    den = den + b
            with np.errstate(all="ignore"):
                out[i, j] = T(np.float64(num) / np.float64(den))
    return out


# ---- the guided filter -------------------------------------------------------------------------------------------------------------------
def guided_prepare(image, features, noise, T, demodulate):
    """DR.prepare plus the two additions of the guided form -> valid, has, e, n, z, cov, a, v"""
    T = np.dtype(T).type
    noise = np.asarray(noise)
    DR._is(T, noise)
    valid, has, e, n, z, cov, a = DR.prepare(image, features, T, demodulate)
    with np.errstate(all="ignore"):
        valid = valid & np.isfinite(noise)
        has = has & valid
        fl = T(2.0 ** -6)
        L = (e[..., 0] + e[..., 1]) + e[..., 2]
        s = noise * np.where(L > fl, L, fl)
        v = s * s
        v = np.where(v > T(V_MIN), v, T(V_MIN))
        v = np.where(v < T(V_MAX), v, T(V_MAX))
    DR._is(T, L, s, v)
    return valid, has, e, n, z, cov, a, v


def guided_level(e, valid, has, n, z, cov, v, k, m, sigma_color, sigma_depth, T):
    """DR.level with the colour distance divided by the CENTRE pixel's v"""
    T = np.dtype(T).type
    s = 1 << k
    inv_sc, inv_sz = DR.level_constants(k, sigma_color, sigma_depth, T)
    H, W = valid.shape
    sum_w = np.zeros((H, W), T)
    sum_e = np.zeros((H, W, 3), T)
    with np.errstate(all="ignore"):
        for dj in range(-2, 3):
            for di in range(-2, 3):
                h = T(DR.K[abs(di)] * DR.K[abs(dj)])
                if di == 0 and dj == 0:
                    sum_w = sum_w + h
                    sum_e = sum_e + h * e
                    continue
                ok = DR._shift(valid, s * di, s * dj, False)
                eq = DR._shift(e, s * di, s * dj, T(0))
                nq = DR._shift(n, s * di, s * dj, T(0))
                zq = DR._shift(z, s * di, s * dj, T(0))
                cq = DR._shift(cov, s * di, s * dj, T(0))
                hq = DR._shift(has, s * di, s * dj, False)
                d = e - eq
                dc = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                dc = dc / v
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
                DR._is(T, d, dc, w_c, t_v, w_v, w, dot, t, zs, r, w_z, wg)
                w = np.where(has & hq, wg, w)
                term = w[..., None] * eq
                sum_w = sum_w + np.where(ok, w, T(0))
                sum_e = sum_e + np.where(ok[..., None], term, T(0))
                DR._is(T, w, term, sum_w, sum_e)
        out = sum_e / sum_w[..., None]
    DR._is(T, out)
    return out


def guided(image, features, noise, T, levels=3, m=1, sigma_color=1.0, sigma_depth=0.1, demodulate=True, gamma=1):
    """the guided definition, vectorised -> out [H, W, 3] of type T; NaN where the pixel is not valid"""
    valid, has, e, n, z, cov, a, v = guided_prepare(image, features, noise, T, demodulate)
    for k in range(levels):
        e = guided_level(e, valid, has, n, z, cov, v, k, m, sigma_color, sigma_depth, T)
    return DR.finish(e, a, valid, demodulate, gamma, T)


def guided_scalar(image, features, noise, T, levels=3, m=1, sigma_color=1.0, sigma_depth=0.1, demodulate=True, gamma=1):
    """the guided definition one pixel at a time on numpy scalars of type T (for tiny frames)"""
    T = np.dtype(T).type
    c, f, rho = np.asarray(image), np.asarray(features), np.asarray(noise)
    DR._is(T, c, f, rho)
    H, W = c.shape[:2]
    one, zero, fl = T(1), T(0), T(2.0 ** -6)
    valid = [[bool(np.isfinite(c[i, j]).all() and np.isfinite(f[i, j]).all() and np.isfinite(rho[i, j])) for j in range(W)] for i in range(H)]
    has = [[valid[i][j] and bool(f[i, j, 7] > zero) for j in range(W)] for i in range(H)]
    n = [[(zero, zero, zero)] * W for _ in range(H)]
    z = [[zero] * W for _ in range(H)]
    a = [[(one, one, one)] * W for _ in range(H)]
    e = [[None] * W for _ in range(H)]
    v = [[one] * W for _ in range(H)]
    with np.errstate(all="ignore"):
        for i in range(H):
            for j in range(W):
                cv = f[i, j, 7]
                if has[i][j]:
                    n[i][j] = (f[i, j, 3] / cv, f[i, j, 4] / cv, f[i, j, 5] / cv)
                    z[i][j] = f[i, j, 6] / cv
                if demodulate:
                    a[i][j] = tuple(max(f[i, j, k], fl) if valid[i][j] else one for k in range(3))
                    e[i][j] = tuple(c[i, j, k] / a[i][j][k] for k in range(3))
                else:
                    e[i][j] = tuple(c[i, j, k] for k in range(3))
                if valid[i][j]:
                    L = (e[i][j][0] + e[i][j][1]) + e[i][j][2]
                    s = rho[i, j] * (L if L > fl else fl)
                    vv = s * s
                    vv = vv if vv > T(V_MIN) else T(V_MIN)
                    vv = vv if vv < T(V_MAX) else T(V_MAX)
                    assert type(vv) is T
                    v[i][j] = vv
        for lv in range(levels):
            s = 1 << lv
            inv_sc, inv_sz = DR.level_constants(lv, sigma_color, sigma_depth, T)
            nxt = [[None] * W for _ in range(H)]
            for i in range(H):
                for j in range(W):
                    if not valid[i][j]:
                        nxt[i][j] = e[i][j]
                        continue
                    ep, np_, zp, cp, vp = e[i][j], n[i][j], z[i][j], f[i, j, 7], v[i][j]
                    sw, se = zero, [zero, zero, zero]
                    for dj in range(-2, 3):
                        for di in range(-2, 3):
                            h = T(DR.K[abs(di)] * DR.K[abs(dj)])
                            if di == 0 and dj == 0:
                                w, eq = h, ep
                            else:
                                qi, qj = i + s * di, j + s * dj
                                if not (0 <= qi < H and 0 <= qj < W) or not valid[qi][qj]:
                                    continue
                                eq, nq, zq, cq = e[qi][qj], n[qi][qj], z[qi][qj], f[qi, qj, 7]
                                d0, d1, d2 = ep[0] - eq[0], ep[1] - eq[1], ep[2] - eq[2]
                                dc = (d0 * d0 + d1 * d1) + d2 * d2
                                dc = dc / vp
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
                    x = e[i][j][k] * a[i][j][k] if demodulate else e[i][j][k]
                    out[i, j, k] = np.sqrt(x) if gamma else x
    return out


def special_noise(H, W, T, seed):
    """a seeded noise map [H, W] of type T with, in frames of 12 pixels or more, the special values of the definition: 0, a value below
    the root of V_MIN (its square clamps to V_MIN), a huge value (its square overflows binary32 and clamps to V_MAX), NaN, +inf, and one
    of them on the border"""
    T = np.dtype(T).type
    rng = np.random.default_rng(seed)
    m = (2.0 ** rng.uniform(-6, 3, size=(H, W))).astype(T)
    if H * W >= 12:
        pix = [(0, 0)]
        while len(pix) < 5:
            pq = (int(rng.integers(H)), int(rng.integers(W)))
            if pq not in pix:
                pix.append(pq)
        for pq, val in zip(pix, (0.0, 2.0 ** -30, 3.0e25, np.nan, np.inf)):
            m[pq] = val
    return m


# ---- tile-prefix features ----------------------------------------------------------------------------------------------------------------
def tile_mask(t, width, height):
    tiles_i = (height + 7) // 8
    tj, ti = divmod(int(t), tiles_i)
    mk = np.zeros((height, width), bool)
    mk[ti * 8:ti * 8 + 8, tj * 8:tj * 8 + 8] = True
    return mk


def chunk_mask(chunks, c, width, height):
    """bool [H, W]: the pixels of the tiles with C_t == c"""
    mk = np.zeros((height, width), bool)
    for t in np.flatnonzero(np.asarray(chunks) == c):
        mk |= tile_mask(t, width, height)
    return mk


def tile_prefix_features(it, T, chunks, width, height):
    """``it``: features_ref.items of the whole render -> raw [H, W, 8]: tile t holds features_ref.resolve over the chunks [0, C_t)"""
    out = np.zeros((height, width, FR.CHANNELS), np.dtype(T).type)
    for c in sorted(set(int(x) for x in chunks)):
        raw, _ = FR.resolve(it, T, (0, c))
        mk = chunk_mask(chunks, c, width, height)
        out[mk] = raw[mk]
    return out


# ---- an adaptive accumulator from oracle samples (the way tests/test_gpu_adaptive.py builds its case, restated) -----------------------------
def _fx(x):
    """one radiance as the kernel adds it (64.64, truncated towards zero) as a Python integer; None: it poisons the pixel"""
    x = float(x)
    if not (abs(x) < 2147483648.0):
        return None
    mt, ex = math.frexp(abs(x))
    mant, sh = int(mt * 2 ** 53), ex - 53 + 64
    val = mant << sh if sh >= 0 else mant >> -sh
    return -val if x < 0 else val


def _q(fx):
    return 0 if fx is None or fx < 0 else min(fx >> 40, 2 ** 30 - 1)


def oracle_words(samples, chunk_spp, counts):
    """samples[i, j, k, c] (float64, sample order) -> {n: words[i, j, 8] after the first n samples}: sums, poison count, half difference"""
    H, W, S, _ = samples.shape
    out = {n: np.zeros((H, W, 8), np.uint64) for n in counts}
    for i in range(H):
        for j in range(W):
            sums, poison, h = [0, 0, 0], 0, 0
            for k in range(S):
                odd = (k // chunk_spp) & 1
                for c in range(3):
                    fx = _fx(samples[i, j, k, c])
                    if fx is None:
                        poison += 1
                    else:
                        sums[c] += fx
                        h += -_q(fx) if odd else _q(fx)
                if k + 1 in out:
                    w = out[k + 1][i, j]
                    for c in range(3):
                        w[2 * c], w[2 * c + 1] = AW.split128(sums[c])
                    w[6], w[7] = poison, h & AW.M64
    return out


def rule_decisions(words, width, height, n, tol, floor):
    """converged[t] by the written rule (accum_words.decisions with no deviation)"""
    return AW.decisions(words, width, height, n, tol, floor)


def rule_chunks(words_at, checkpoints, n_chunks, chunk_spp, width, height, tol, floor):
    """C_t by the written rule from {c: words after the chunks [0, c)}"""
    n_tiles = ((height + 7) // 8) * ((width + 7) // 8)
    ct = np.full(n_tiles, n_chunks, np.int32)
    for c in reversed(checkpoints):
        ct[rule_decisions(words_at[c], width, height, c * chunk_spp, tol, floor)] = c
    return ct


def adaptive_words(words_at, chunks, width, height):
    """the words of the adaptive accumulator: tile t's pixels from words_at[C_t]"""
    out = np.zeros((height, width, 8), np.uint64)
    for c in sorted(set(int(x) for x in chunks)):
        mk = chunk_mask(chunks, c, width, height)
        out[mk] = words_at[c][mk]
    return out


# ---- hand-made words for the noise map ---------------------------------------------------------------------------------------------------
NW, NH, NSPP, NCS = 11, 13, 20, 3
NCHUNKS = [2, 4, 6, 8]                           # the 2 x 2 tiles of 13 rows x 11 columns hold n = 6, 12, 18 and, capped, 20 samples


def noise_cases():
    """-> [(name, words, floor, {(i, j): expected binary64 value or None for NaN})] on a frame of 13 rows x 11 columns whose four tiles hold
    6, 12, 18 and 20 samples.  Every expectation is spelled out by hand: rho = |H| 2^-24 / max(max(y, 0), floor n), then the 3 x 3 binomial
    mean over the neighbours inside the frame that are not poisoned (weights 4 centre, 2 edge, 1 corner)."""
    cases = []
    # a negative H in the frame's corner: D = 6, M = 1 * 6 -> rho = 1 there, 0 elsewhere.  Corner pixel: taps 4 + 2 + 2 + 1 = 9
    w = AW.make_words(NW, NH)
    AW.set_pixel(w, 0, 0, h=-(6 << 24))
    cases.append(("negative_h_in_the_corner", w, 1.0, {(0, 0): 4.0 / 9.0, (1, 0): 2.0 / 12.0, (1, 1): 1.0 / 16.0, (0, 2): 0.0, (2, 2): 0.0}))
    # H = INT64_MIN: |H| = 2^63, D = 2^39 = y -> rho = 1 (floor 0); an interior pixel: 4 / 16
    w = AW.make_words(NW, NH)
    AW.set_pixel(w, 4, 4, rgb=(AW.U(1 << 39), 0, 0), h=-(1 << 63))
    cases.append(("h_most_negative", w, 0.0, {(4, 4): 0.25, (3, 4): 0.125, (5, 5): 0.0625, (4, 6): 0.0}))
    # floor = 0 and y = 0: M = 0 -> rho = 0 whatever H says; y < 0 the same
    w = AW.make_words(NW, NH)
    AW.set_pixel(w, 4, 4, h=1 << 40)
    AW.set_pixel(w, 5, 4, rgb=(-AW.U(3), 0, 0), h=1 << 40)
    cases.append(("floor_0_and_y_0", w, 0.0, {(4, 4): 0.0, (5, 4): 0.0, (4, 5): 0.0}))
    # a poisoned centre is NaN; a poisoned neighbour is left out of both sums: at (4, 5) the taps are 16 - 2 = 14 and rho = 1 at (3, 5)
    w = AW.make_words(NW, NH)
    AW.set_pixel(w, 4, 4, rgb=(AW.U(5), 0, 0), h=1 << 50, poison=2)
    AW.set_pixel(w, 3, 5, rgb=(AW.U(6), 0, 0), h=6 << 24)
    cases.append(("poisoned_centre_and_neighbour", w, 0.0, {(4, 4): None, (4, 5): 2.0 / 14.0, (3, 5): 4.0 / 15.0, (3, 6): 2.0 / 16.0}))
    # neighbouring tiles with different C_t: rows 7 and 8 of column 0 lie in tiles 0 (n = 6) and 1 (n = 12); the same H = 6 gives rho 1 and 1/2
    w = AW.make_words(NW, NH)
    AW.set_pixel(w, 7, 0, h=6 << 24)
    AW.set_pixel(w, 8, 0, h=-(6 << 24))
    cases.append(("tiles_with_different_chunk_counts", w, 1.0, {(7, 0): (4.0 * 1.0 + 2.0 * 0.5) / 12.0, (8, 0): (2.0 * 1.0 + 4.0 * 0.5) / 12.0,
                                                                (7, 1): (2.0 * 1.0 + 1.0 * 0.5) / 16.0}))
    # the ragged last tile row and column: the frame's last pixel lies in tile 3 (n = min(20, 8 * 3) = 20): D = 20 = M
    w = AW.make_words(NW, NH)
    AW.set_pixel(w, 12, 10, h=20 << 24)
    AW.set_pixel(w, 12, 0, h=12 << 24)               # tile 1: n = 12
    cases.append(("ragged_last_tile_row", w, 1.0, {(12, 10): 4.0 / 9.0, (11, 9): 1.0 / 16.0, (12, 0): 4.0 / 9.0, (12, 1): 2.0 / 12.0}))
    return cases
