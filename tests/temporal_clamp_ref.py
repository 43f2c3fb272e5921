"""The witness of the temporal clamp (include/rtw_hip.h rtw_clamped_step_*): the clamped step restated in numpy twice -- vectorised with the
element type of every intermediate asserted, and one pixel and one numpy scalar at a time.  Nothing of the product is used but its camera
mirror; the frame is prepared by the denoiser's witness (denoise_ref.prepare), the host constants are temporal_ref's and the plain steps it is
compared with are temporal_ref.step / temporal_noise_ref.step_moments.  numpy rounds every operation once and never fuses.

    step_clamped(image, features, cam, T, state, cam_prev, moment, moments, clamp, ...)   vectorised -> (out, next state, next moment plane or None)
    step_clamped_scalar(...)                                                              the same definition one pixel at a time
    window_bounds(valid, has, e, n, z, cov, T, radius, guides, sigma, m, sigma_depth)     the window of the current frame -> (lo, hi) [H, W, 3]
    clamp_constants(T, sigma, len_scale)                                                  what the host rounds to T
    census(...)                                                                           which regimes of the definition a step reaches
    no_movement_sequence / constant_sequence                                              the inputs of two properties of the definition
A clamp is a dict of radius, guides, sigma, len_scale (CLAMP_DEFAULTS); states and moment planes are temporal_ref's and temporal_noise_ref's.
Arrays are indexed [i, j] (row, column): the library's memory is the transpose, pixel (i, j) at j*H + i."""
import numpy as np

import denoise_ref as DR
import temporal_noise_ref as NR
import temporal_ref as TR

CLAMP_DEFAULTS = dict(radius=1, guides=False, sigma=1.0, len_scale=1.0)
_is = DR._is
bits, same_bits = DR.bits, DR.same_bits

#: the tile of the kernel (rows x columns); the frames (W, H) of tests/test_gpu_temporal_clamp.py -- the last is one tile plus one row and one column
TILE = (32, 8)
SIZES = [(1, 1), (3, 2), (70, 40), (64, 36), (9, 33)]
SEEDS = {np.float32: 61, np.float64: 62}


def clamp_constants(T, sigma, len_scale):
    """what the host computes in binary64 -> (ks, ls) of type T"""
    T = np.dtype(T).type
    return T(np.float64(sigma)), T(np.float64(len_scale))


def _clamp(clamp):
    ck = dict(CLAMP_DEFAULTS)
    ck.update(clamp or {})
    assert set(ck) == set(CLAMP_DEFAULTS), sorted(ck)
    return ck


def window_bounds(valid, has, e, n, z, cov, T, radius, guides, sigma, m, sigma_depth, details=None):
    """the window of the current frame, vectorised: whole frames per tap -> (lo, hi), [H, W, 3] of type T (NaN where S0 = 0)"""
    T = np.dtype(T).type
    H, W = valid.shape
    one, zero = T(1), T(0)
    ks = T(np.float64(sigma))
    with np.errstate(all="ignore"):
        inv_sz = T(np.float64(1.0) / np.float64(float(sigma_depth) * float(sigma_depth)))
        S0, S1, S2 = np.zeros((H, W), T), np.zeros((H, W, 3), T), np.zeros((H, W, 3), T)
        n_taps, n_invalid, n_mixed = (np.zeros((H, W), np.int64) for _ in range(3))
        cut = np.zeros((H, W, 4), bool)
        for dj in range(-radius, radius + 1):
            for di in range(-radius, radius + 1):
                ii, jj = np.arange(H)[:, None] + di, np.arange(W)[None, :] + dj
                inside = (ii >= 0) & (ii < H) & (jj >= 0) & (jj < W)
                ok = DR._shift(valid, di, dj, False)
                eq, nq, zq, cq = DR._shift(e, di, dj, zero), DR._shift(n, di, dj, zero), DR._shift(z, di, dj, zero), DR._shift(cov, di, dj, zero)
                sq = eq * eq
                if guides:
                    t_v = one - np.abs(cov - cq)
                    w = np.where(t_v > zero, t_v, zero)
                    dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    tt = np.where(dot > zero, dot, zero)
                    for _ in range(m):
                        tt = tt * tt
                    zs = z + zq
                    r = (z - zq) / np.where(zs > zero, zs, one)
                    w_z = one / (one + (r * r) * inv_sz)
                    wg = (w * tt) * w_z
                    w = np.where(has & (cq > zero), wg, w)
                    t1, t2 = w[..., None] * eq, w[..., None] * sq
                    _is(T, t_v, dot, tt, zs, r, w_z, wg, w, t1, t2)
                    S0 = S0 + np.where(ok, w, zero)
                else:
                    t1, t2 = eq, sq
                    S0 = S0 + np.where(ok, one, zero)
                S1 = S1 + np.where(ok[..., None], t1, zero)
                S2 = S2 + np.where(ok[..., None], t2, zero)
                _is(T, sq, S0, S1, S2)
                n_taps += ok
                n_invalid += inside & ~ok
                n_mixed += ok & (has != (cq > zero))
                cut[..., 0] |= ii < 0
                cut[..., 1] |= ii >= H
                cut[..., 2] |= jj < 0
                cut[..., 3] |= jj >= W
        mu = S1 / S0[..., None]
        vt = S2 / S0[..., None] - mu * mu
        var = np.where(vt > zero, vt, zero)
        sd = np.sqrt(var)
        dlt = ks * sd
        lo, hi = mu - dlt, mu + dlt
        _is(T, mu, vt, var, sd, dlt, lo, hi)
    if details is not None:
        details.update(S0=S0, sd=sd, n_taps=n_taps, n_invalid=n_invalid, n_mixed=n_mixed, cut=cut)
    return lo, hi


def step_clamped(image, features, cam, T, state=None, cam_prev=None, moment=None, moments=None, clamp=None, m=1, sigma_depth=0.1, min_weight=0.25, history_max=16.0,
                 demodulate=True, gamma=1, details=None):
    """the definition, vectorised -> (out [H, W, 3], the next state, the next moment plane -- None without moments).  `moments` defaults to
    whether a moment plane is given; the first frame is the plain step's."""
    T = np.dtype(T).type
    ck = _clamp(clamp)
    if moments is None:
        moments = moment is not None
    assert (state is None) == (cam_prev is None) and (moment is None or (moments and state is not None)) and not (moments and state is not None and moment is None)
    valid, has, e, n, z, cov, a = DR.prepare(image, features, T, demodulate)
    H, W = valid.shape
    K = TR.host_constants(cam_prev, T, sigma_depth, min_weight, history_max)
    ks, ls = clamp_constants(T, ck["sigma"], ck["len_scale"])
    one, zero = T(1), T(0)
    with np.errstate(all="ignore"):
        y = (e[..., 0] + e[..., 1]) + e[..., 2]
        y2 = y * y
        _is(T, y, y2)
        if state is None:
            accept = np.zeros((H, W), bool)
            en, ln, mn = e.copy(), np.ones((H, W), T), y2.copy()
        else:
            Ep, Gp, Lp = state["E"], state["G"], state["L"]
            Mp = np.asarray(moment) if moments else np.zeros((H, W), T)
            _is(T, Ep, Gp, Lp, Mp)
            # ---- the window of the current frame
            dw_ = {}
            lo, hi = window_bounds(valid, has, e, n, z, cov, T, ck["radius"], ck["guides"], ck["sigma"], m, sigma_depth, details=dw_)
            # ---- the pixel's own ray, the projection: the plain step's
            o, llc, hor, ver = TR._cam_fields(cam, T, ("origin", "lower_left_corner", "horizontal", "vertical"))
            po, pw, ph, pv = TR._cam_fields(cam_prev, T, ("origin", "w", "horizontal", "vertical"))
            su = (np.arange(W, dtype=np.int64).astype(T) + T(1.5)) / T(W)
            tv = ((H - np.arange(H, dtype=np.int64)).astype(T) - T(0.5)) / T(H)
            D = [((llc[k] + su * hor[k])[None, :] + (tv * ver[k])[:, None]) - o[k] for k in range(3)]
            sl = np.sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2])
            nD = [D[k] / sl for k in range(3)]
            d = [np.where(has, (o[k] + z * nD[k]) - po[k], nD[k]) for k in range(3)]
            dot3 = lambda v: (d[0] * v[0] + d[1] * v[1]) + d[2] * v[2]
            dw = dot3(pw)
            front = dw < zero
            lam = K["Kw"] / dw
            s = (lam * dot3(ph) - K["Qh"]) * K["ih"]
            t = (lam * dot3(pv) - K["Qv"]) * K["iv"]
            x = s * T(W) - T(1.5)
            yy = (T(H) - T(0.5)) - t * T(H)
            inr = (x > T(-1)) & (x < T(W)) & (yy > T(-1)) & (yy < T(H))
            xs, ys = np.where(inr, x, zero), np.where(inr, yy, zero)
            xf, yf = np.floor(xs), np.floor(ys)
            x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
            fx, fy = xs - xf, ys - yf
            zexp = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            _is(T, su, tv, sl, *D, *nD, *d, dw, lam, s, t, x, yy, fx, fy, zexp)
            # ---- the taps of the previous state
            valid_q = ~np.isnan(Gp[..., 3])
            sum_w, sum_l, sum_m, sum_e = np.zeros((H, W), T), np.zeros((H, W), T), np.zeros((H, W), T), np.zeros((H, W, 3), T)
            for b in (0, 1):
                kx = fx if b else one - fx
                for c in (0, 1):
                    ky = fy if c else one - fy
                    sb = ky * kx
                    qi, qj = y0 + c, x0 + b
                    inside = (qi >= 0) & (qi < H) & (qj >= 0) & (qj < W)
                    gi, gj = np.clip(qi, 0, H - 1), np.clip(qj, 0, W - 1)
                    ok = inside & valid_q[gi, gj]
                    eq, gq, lq, mq = Ep[gi, gj], Gp[gi, gj], Lp[gi, gj], Mp[gi, gj]
                    t_v = one - np.abs(cov - gq[..., 3])
                    w_v = np.where(t_v > zero, t_v, zero)
                    w = sb * w_v
                    dot = (n[..., 0] * gq[..., 0] + n[..., 1] * gq[..., 1]) + n[..., 2] * gq[..., 2]
                    tt = np.where(dot > zero, dot, zero)
                    for _ in range(m):
                        tt = tt * tt
                    zs = zexp + eq[..., 3]
                    r = (zexp - eq[..., 3]) / np.where(zs > zero, zs, one)
                    w_z = one / (one + (r * r) * K["inv_sz"])
                    wg = (w * tt) * w_z
                    w = np.where(has & (gq[..., 3] > zero), wg, w)
                    term, lterm, mterm = w[..., None] * eq[..., 0:3], w * lq, w * mq
                    _is(T, sb, t_v, w_v, dot, tt, zs, r, w_z, wg, w, term, lterm, mterm)
                    sum_w = sum_w + np.where(ok, w, zero)
                    sum_e = sum_e + np.where(ok[..., None], term, zero)
                    sum_l = sum_l + np.where(ok, lterm, zero)
                    sum_m = sum_m + np.where(ok, mterm, zero)
                    _is(T, sum_w, sum_e, sum_l, sum_m)
            accept = front & inr & (sum_w >= K["w_min"])
            eh = sum_e / sum_w[..., None]
            lh = sum_l / sum_w
            # ---- the clamp (a NaN bound fails both comparisons), then the plain blend on hc and lh'
            below, above = eh < lo, eh > hi
            hc = np.where(below, lo, np.where(above, hi, eh))
            moved = (hc != eh).any(axis=-1)
            lc = np.where(moved, lh * ls, lh)
            l1 = lc + one
            nn = np.where(l1 < K["n_max"], l1, K["n_max"])
            alpha = one / nn
            eb = hc + alpha[..., None] * (e - hc)
            mh = sum_m / sum_w
            mb = mh + alpha * (y2 - mh)
            _is(T, eh, lh, hc, lc, l1, nn, alpha, eb, mh, mb)
            en = np.where(accept[..., None], eb, e)
            ln = np.where(accept, nn, one)
            mn = np.where(accept, mb, y2)
            if details is not None:
                details.update(dw_, front=front, inr=inr, below=below, above=above, moved=moved, lo=lo, hi=hi, eh=eh, hc=hc, lh=lh, lc=lc)
        out = en * a if demodulate else en.copy()
        if gamma:
            out = np.sqrt(out)
    _is(T, en, ln, mn, out)
    out[~valid] = np.nan
    nxt = TR.empty_state(H, W, T)
    nxt["E"][..., 0:3] = np.where(valid[..., None], en, zero)
    nxt["E"][..., 3] = z
    nxt["G"][..., 0:3] = n
    nxt["G"][..., 3] = np.where(valid, cov, T(np.nan))
    nxt["L"][...] = np.where(valid, ln, zero)
    M = np.where(valid, mn, zero) if moments else None
    if details is not None:
        details.update(valid=valid, has=has, accept=accept, first=state is None)
    return out, nxt, M


def step_clamped_scalar(image, features, cam, T, state=None, cam_prev=None, moment=None, moments=None, clamp=None, m=1, sigma_depth=0.1, min_weight=0.25, history_max=16.0,
                        demodulate=True, gamma=1):
    """the same definition, one pixel at a time on numpy scalars of type T (for small frames)"""
    T = np.dtype(T).type
    ck = _clamp(clamp)
    if moments is None:
        moments = moment is not None
    assert (state is None) == (cam_prev is None)
    c, f = np.asarray(image), np.asarray(features)
    _is(T, c, f)
    H, W = c.shape[:2]
    K = TR.host_constants(cam_prev, T, sigma_depth, min_weight, history_max)
    ks, ls = clamp_constants(T, ck["sigma"], ck["len_scale"])
    R = ck["radius"]
    one, zero, floor_ = T(1), T(0), T(2.0 ** -6)
    out = np.full((H, W, 3), np.nan, T)
    nxt = TR.empty_state(H, W, T)
    nxt["G"][..., 3] = np.nan
    M = np.zeros((H, W), T)
    dot3 = lambda u, v: (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]

    def prep(i, j):
        """Prepare for one pixel -> None (not valid) or (cov, has, n, z, a, e)"""
        if not bool(np.isfinite(c[i, j]).all() and np.isfinite(f[i, j]).all()):
            return None
        cov = f[i, j, 7]
        has = bool(cov > zero)
        n = (f[i, j, 3] / cov, f[i, j, 4] / cov, f[i, j, 5] / cov) if has else (zero, zero, zero)
        z = f[i, j, 6] / cov if has else zero
        a = tuple(max(f[i, j, k], floor_) for k in range(3)) if demodulate else (one, one, one)
        e = tuple(c[i, j, k] / a[k] for k in range(3)) if demodulate else tuple(c[i, j, k] for k in range(3))
        return cov, has, n, z, a, e

    if state is not None:
        o, llc, hor, ver = TR._cam_fields(cam, T, ("origin", "lower_left_corner", "horizontal", "vertical"))
        po, pw, ph, pv = TR._cam_fields(cam_prev, T, ("origin", "w", "horizontal", "vertical"))
        Ep, Gp, Lp = state["E"], state["G"], state["L"]
        Mp = np.asarray(moment) if moments else np.zeros((H, W), T)
    with np.errstate(all="ignore"):
        P = [[prep(i, j) for j in range(W)] for i in range(H)]
        for i in range(H):
            for j in range(W):
                if P[i][j] is None:
                    continue
                cov, has, n, z, a, e = P[i][j]
                y = (e[0] + e[1]) + e[2]
                y2 = y * y
                en, ln, mn = e, one, y2
                if state is not None:
                    su = (np.int64(j).astype(T) + T(1.5)) / T(W)
                    tv = (np.int64(H - i).astype(T) - T(0.5)) / T(H)
                    D = [((llc[k] + su * hor[k]) + tv * ver[k]) - o[k] for k in range(3)]
                    sl = np.sqrt(dot3(D, D))
                    nD = [D[k] / sl for k in range(3)]
                    d = [(o[k] + z * nD[k]) - po[k] for k in range(3)] if has else nD
                    dw = dot3(d, pw)
                    front = bool(dw < zero)
                    lam = K["Kw"] / dw
                    s = (lam * dot3(d, ph) - K["Qh"]) * K["ih"]
                    t = (lam * dot3(d, pv) - K["Qv"]) * K["iv"]
                    x = s * T(W) - T(1.5)
                    yy = (T(H) - T(0.5)) - t * T(H)
                    inr = bool(x > T(-1) and x < T(W) and yy > T(-1) and yy < T(H))
                    if front and inr:                           # (otherwise the pixel resets: the window decides nothing)
                        xf, yf = np.floor(x), np.floor(yy)
                        x0, y0 = int(xf), int(yf)
                        fx, fy = x - xf, yy - yf
                        zexp = np.sqrt(dot3(d, d))
                        sw, sl_, sm, se = zero, zero, zero, [zero, zero, zero]
                        for b in (0, 1):
                            kx = fx if b else one - fx
                            for cc in (0, 1):
                                ky = fy if cc else one - fy
                                sb = ky * kx
                                qi, qj = y0 + cc, x0 + b
                                if not (0 <= qi < H and 0 <= qj < W) or bool(np.isnan(Gp[qi, qj, 3])):
                                    continue
                                eq, gq, lq, mq = Ep[qi, qj], Gp[qi, qj], Lp[qi, qj], Mp[qi, qj]
                                t_v = one - abs(cov - gq[3])
                                w = sb * (t_v if t_v > zero else zero)
                                if has and bool(gq[3] > zero):
                                    dot = (n[0] * gq[0] + n[1] * gq[1]) + n[2] * gq[2]
                                    tt = dot if dot > zero else zero
                                    for _ in range(m):
                                        tt = tt * tt
                                    zs = zexp + eq[3]
                                    r = (zexp - eq[3]) / (zs if zs > zero else one)
                                    w = (w * tt) * (one / (one + (r * r) * K["inv_sz"]))
                                assert type(w) is T
                                sw = sw + w
                                sl_ = sl_ + w * lq
                                sm = sm + w * mq
                                for k in range(3):
                                    se[k] = se[k] + w * eq[k]
                        if bool(sw >= K["w_min"]):
                            # ---- the window of the current frame
                            S0, S1, S2 = zero, [zero, zero, zero], [zero, zero, zero]
                            for dj in range(-R, R + 1):
                                for di in range(-R, R + 1):
                                    qi, qj = i + di, j + dj
                                    if not (0 <= qi < H and 0 <= qj < W) or P[qi][qj] is None:
                                        continue
                                    cq, hq, nq, zq, _, eq = P[qi][qj]
                                    if ck["guides"]:
                                        t_v = one - abs(cov - cq)
                                        w = t_v if t_v > zero else zero
                                        if has and bool(cq > zero):
                                            dot = (n[0] * nq[0] + n[1] * nq[1]) + n[2] * nq[2]
                                            tt = dot if dot > zero else zero
                                            for _ in range(m):
                                                tt = tt * tt
                                            zs = z + zq
                                            r = (z - zq) / (zs if zs > zero else one)
                                            w = (w * tt) * (one / (one + (r * r) * K["inv_sz"]))
                                        assert type(w) is T
                                        S0 = S0 + w
                                        for k in range(3):
                                            S1[k] = S1[k] + w * eq[k]
                                            S2[k] = S2[k] + w * (eq[k] * eq[k])
                                    else:
                                        S0 = S0 + one
                                        for k in range(3):
                                            S1[k] = S1[k] + eq[k]
                                            S2[k] = S2[k] + eq[k] * eq[k]
                            eh = [se[k] / sw for k in range(3)]
                            lh = sl_ / sw
                            hc, moved = [None] * 3, False
                            for k in range(3):
                                mu = S1[k] / S0
                                vt = S2[k] / S0 - mu * mu
                                sd = np.sqrt(vt if vt > zero else zero)
                                lo, hi = mu - ks * sd, mu + ks * sd
                                assert type(lo) is T and type(hi) is T
                                hc[k] = lo if eh[k] < lo else (hi if eh[k] > hi else eh[k])
                                moved = moved or bool(hc[k] != eh[k])
                            if moved:
                                lh = lh * ls
                            l1 = lh + one
                            nn = l1 if l1 < K["n_max"] else K["n_max"]
                            alpha = one / nn
                            en = tuple(hc[k] + alpha * (e[k] - hc[k]) for k in range(3))
                            ln = nn
                            mh = sm / sw
                            mn = mh + alpha * (y2 - mh)
                            assert type(mn) is T and type(alpha) is T and all(type(v) is T for v in en)
                for k in range(3):
                    v = en[k] * a[k] if demodulate else en[k]
                    out[i, j, k] = np.sqrt(v) if gamma else v
                    nxt["E"][i, j, k] = en[k]
                    nxt["G"][i, j, k] = n[k]
                nxt["E"][i, j, 3] = z
                nxt["G"][i, j, 3] = cov
                nxt["L"][i, j] = ln
                M[i, j] = mn
    return out, nxt, (M if moments else None)


def same_step(got, ref):
    """two results (out, state, moment plane or None) agree on the bits"""
    return same_bits(got[0], ref[0]) and TR.same_state(got[1], ref[1]) and ((got[2] is None and ref[2] is None) or same_bits(got[2], ref[2]))


def census(image, features, cam, T, state, cam_prev, moment=None, clamp=None, **params):
    """which regimes of the definition one clamped step reaches, counted on the witness alone.  (Counts over accepted pixels unless said
    otherwise: the clamp decides nothing anywhere else.)"""
    T = np.dtype(T).type
    ck = _clamp(clamp)
    d = {}
    step_clamped(image, features, cam, T, state, cam_prev, moment, clamp=ck, details=d, **params)
    v = d["valid"]
    H, W = v.shape
    if d["first"]:
        return dict(first_frame=int(v.sum()), accepted=0)
    acc = v & d["accept"]
    r = ck["radius"]
    nan_b = np.isnan(d["lo"]).any(axis=-1)
    with np.errstate(all="ignore"):
        return dict(first_frame=0,
                    accepted=int(acc.sum()),
                    reset=int((v & ~d["accept"]).sum()),
                    clamped_lo=int((acc & d["below"].any(axis=-1)).sum()),
                    clamped_hi=int((acc & d["above"].any(axis=-1)).sum()),
                    untouched=int((acc & ~d["moved"]).sum()),
                    nan_bounds=int((acc & nan_b & (d["S0"] == 0)).sum()),
                    sd_zero=int((acc & ~nan_b & (d["sd"] == 0).any(axis=-1)).sum()),
                    cut_top=int((acc & d["cut"][..., 0]).sum()), cut_bottom=int((acc & d["cut"][..., 1]).sum()),
                    cut_left=int((acc & d["cut"][..., 2]).sum()), cut_right=int((acc & d["cut"][..., 3]).sum()),
                    frame_smaller_than_window=int(H < 2 * r + 1 or W < 2 * r + 1) * int(acc.sum()),
                    invalid_neighbour=int((acc & (d["n_invalid"] > 0)).sum()),
                    invalid_centre=int((~v).sum()),
                    sky_covered_pair=int((acc & (d["n_mixed"] > 0)).sum()),
                    len_shortened=int((acc & d["moved"] & (bits(d["lc"]) != bits(d["lh"]))).sum()))


def no_movement_sequence(H, W, T, rtw=None):
    """-> (cam, cam_prev, image, features, state, moment): a step the clamp cannot move.  Both cameras are the same, every pixel is a surface at
    one depth with one normal and full coverage, the frame is one colour (powers of two per channel, albedo 1/2) and the history holds exactly
    the frame's (de)modulated colour: every window has mu = e exactly and sd = 0, every gathered eh = e (a weighted mean of equal powers of
    two that survives its roundings or not -- see the test, which asserts on the witness that nothing moved)."""
    if rtw is None:
        import rtw_amd as rtw
    T = np.dtype(T).type
    cam = TR.make_camera(rtw, T, (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), W, H)
    image = np.empty((H, W, 3), T)
    image[...] = np.array([0.25, 0.5, 1.0], T)
    feat = np.zeros((H, W, 8), T)
    feat[..., 0:3] = T(0.5)
    feat[..., 3:8] = np.array([0.0, 0.0, 1.0, 4.0, 1.0], T)
    _, state = TR.step(image, feat, cam, T)
    state["L"][...] = (1 + (np.arange(H)[:, None] + np.arange(W)[None, :]) % 7).astype(T)
    E = state["E"]
    Lm = (E[..., 0] + E[..., 1]) + E[..., 2]
    return cam, cam, image, feat, state, (Lm * Lm).astype(T)


def planted_sequence(T, rtw=None, H=9, W=12):
    """-> (cam, cam_prev, image, features, state, moment): a 12 x 9 step under identical cameras (every pixel reprojects onto itself, so
    every edge has accepted pixels) with the regimes the hand-made sequences do not reach planted by hand.  The base is
    no_movement_sequence's constant surface (sd = 0 exactly).  Planted: columns 8.. of the frame vary (sd > 0); history colours of 2 and of
    0 (clamped at hi and at lo); at (4, 5) a pixel of coverage 1/2 whose normal is the zero vector among covered neighbours, over a
    history that is sky there -- with guides every window weight is 0, so S0 = 0 and the bounds are NaN, while the history is accepted
    with sum_w = 1/2; a sky pixel at (8, 1) over a sky history (sky / covered pairs); a NaN pixel at (1, 9)."""
    T = np.dtype(T).type
    cam, _, image, feat, state, _ = no_movement_sequence(H, W, T, rtw)
    rng = np.random.default_rng(7)
    image[:, 8:] = rng.uniform(0.1, 0.9, (H, W - 8, 3)).astype(T)
    state["E"][2, 1, 0:3] = T(2.0)
    state["E"][6, 10, 0:3] = T(2.0)
    state["E"][5, 1, 0:3] = T(0.0)
    state["E"][3, 9, 0:3] = T(0.0)
    feat[4, 5, 3:8] = np.array([0.0, 0.0, 0.0, 2.0, 0.5], T)
    for i in range(3, 6):
        for j in range(4, 7):
            state["G"][i, j] = 0
            state["E"][i, j, 3] = 0
    feat[8, 1, 3:8] = 0
    state["G"][8, 1] = 0
    state["E"][8, 1, 3] = 0
    image[1, 9, 1] = np.nan
    E = state["E"]
    Lm = (E[..., 0] + E[..., 1]) + E[..., 2]
    return cam, cam, image, feat, state, (Lm * Lm * T(1.5)).astype(T)


def constant_sequence(H, W, T, rtw=None):
    """-> (cam, cam_prev, image, features, state): a constant frame of 0.5 (albedo 1: e = 0.5 with or without demodulation) over a history of
    2.0 everywhere"""
    cam, _, image, feat, state, _ = no_movement_sequence(H, W, T, rtw)
    image[...] = T(0.5)
    feat[..., 0:3] = T(1)
    state["E"][..., 0:3] = T(2.0)
    return cam, cam, image, feat, state
