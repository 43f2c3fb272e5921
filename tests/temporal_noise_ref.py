"""The witness of the temporal moments (include/rtw_hip.h rtw_history_moments_*, rtw_history_noise_device_*): the step with second moments and
the noise map restated in numpy, each twice -- vectorised with the element type of every intermediate asserted, and one pixel and one numpy
scalar at a time.  Nothing of the product is used but its camera mirror; the frame is prepared by the denoiser's witness (denoise_ref.prepare)
and the host constants are temporal_ref's.  numpy rounds every operation once and never fuses.

    step_moments(image, features, cam, T, state, moment, cam_prev, ...)          vectorised -> (out, next state, next moment plane)
    step_moments_scalar(...)                                                     the same definition one pixel at a time
    noise_map(state, moment, T, radius, m, sigma_depth, min_len)                 vectorised -> the map [H, W]
    noise_map_scalar(...)                                                        one pixel at a time
    pack_moment(M, T) / unpack_moment(flat, H, W)                                a moment plane <-> the library's memory
    handmade_moment(state, T, seed)                                              a hand-made previous moment plane for a hand-made state
    census(...)                                                                  which regimes of the two definitions a step and its map reach
A moment plane is an array M [H, W]; states are temporal_ref's dicts.  Arrays are indexed [i, j] (row, column): the library's memory is the
transpose, pixel (i, j) at j*H + i."""
import numpy as np

import denoise_ref as DR
import temporal_ref as TR

NOISE_DEFAULTS = dict(radius=2, m=1, sigma_depth=0.1, min_len=4.0)
_is = DR._is
bits, same_bits = DR.bits, DR.same_bits

#: the frames (W, H) of tests/test_gpu_temporal_noise.py and the committed seeds of their hand-made sequences
SIZES = [(1, 1), (3, 2), (70, 40), (64, 36)]
SEEDS = {np.float32: 51, np.float64: 52}


def moment_elems(H, W, T):
    """elements of T in a packed moment plane: W*H of them, rounded up to 16 bytes"""
    eb = np.dtype(T).itemsize
    return ((W * H * eb + 15) // 16 * 16) // eb


def pack_moment(M, T):
    H, W = M.shape
    flat = np.zeros(moment_elems(H, W, T), T)
    flat[:W * H] = np.swapaxes(M, 0, 1).reshape(-1)
    return flat


def unpack_moment(flat, H, W):
    return np.swapaxes(flat[:W * H].reshape(W, H), 0, 1).copy()


def noise_constants(T, sigma_depth, min_len):
    """what the host computes in binary64 -> (inv_sz, ml) of type T"""
    T = np.dtype(T).type
    with np.errstate(all="ignore"):
        return T(np.float64(1.0) / np.float64(float(sigma_depth) * float(sigma_depth))), T(np.float64(min_len))


# ---- the step with moments ---------------------------------------------------------------------------------------------------------------
def step_moments(image, features, cam, T, state=None, moment=None, cam_prev=None, m=1, sigma_depth=0.1, min_weight=0.25, history_max=16.0, demodulate=True, gamma=1,
                 details=None):
    """the step's definition restated in full (not a call of temporal_ref.step: tests/test_temporal_noise_ref.py compares the two on the
    bits) with the moment plane next to it -> (out, next state, M')"""
    T = np.dtype(T).type
    assert (state is None) == (cam_prev is None) == (moment is None)
    valid, has, e, n, z, cov, a = DR.prepare(image, features, T, demodulate)
    H, W = valid.shape
    K = TR.host_constants(cam_prev, T, sigma_depth, min_weight, history_max)
    one, zero = T(1), T(0)
    with np.errstate(all="ignore"):
        y = (e[..., 0] + e[..., 1]) + e[..., 2]
        y2 = y * y
        _is(T, y, y2)
        if state is None:
            accept = np.zeros((H, W), bool)
            en, ln, mn = e.copy(), np.ones((H, W), T), y2.copy()
        else:
            Ep, Gp, Lp, Mp = state["E"], state["G"], state["L"], np.asarray(moment)
            _is(T, Ep, Gp, Lp, Mp)
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
            l1 = lh + one
            nn = np.where(l1 < K["n_max"], l1, K["n_max"])
            alpha = one / nn
            eb = eh + alpha[..., None] * (e - eh)
            mh = sum_m / sum_w
            mb = mh + alpha * (y2 - mh)
            _is(T, eh, lh, l1, nn, alpha, eb, mh, mb)
            en = np.where(accept[..., None], eb, e)
            ln = np.where(accept, nn, one)
            mn = np.where(accept, mb, y2)
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
    M = np.where(valid, mn, zero)
    _is(T, M)
    if details is not None:
        details.update(valid=valid, has=has, accept=accept, y2=y2)
    return out, nxt, M


def step_moments_scalar(image, features, cam, T, state=None, moment=None, cam_prev=None, m=1, sigma_depth=0.1, min_weight=0.25, history_max=16.0, demodulate=True, gamma=1):
    """the same definition, one pixel at a time on numpy scalars of type T (for small frames)"""
    T = np.dtype(T).type
    assert (state is None) == (cam_prev is None) == (moment is None)
    c, f = np.asarray(image), np.asarray(features)
    _is(T, c, f)
    H, W = c.shape[:2]
    K = TR.host_constants(cam_prev, T, sigma_depth, min_weight, history_max)
    one, zero, floor_ = T(1), T(0), T(2.0 ** -6)
    out = np.full((H, W, 3), np.nan, T)
    nxt = TR.empty_state(H, W, T)
    nxt["G"][..., 3] = np.nan
    M = np.zeros((H, W), T)
    if state is not None:
        o, llc, hor, ver = TR._cam_fields(cam, T, ("origin", "lower_left_corner", "horizontal", "vertical"))
        po, pw, ph, pv = TR._cam_fields(cam_prev, T, ("origin", "w", "horizontal", "vertical"))
        Ep, Gp, Lp, Mp = state["E"], state["G"], state["L"], np.asarray(moment)
    dot3 = lambda u, v: (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]
    with np.errstate(all="ignore"):
        for i in range(H):
            for j in range(W):
                if not bool(np.isfinite(c[i, j]).all() and np.isfinite(f[i, j]).all()):
                    continue
                cov = f[i, j, 7]
                has = bool(cov > zero)
                n = (f[i, j, 3] / cov, f[i, j, 4] / cov, f[i, j, 5] / cov) if has else (zero, zero, zero)
                z = f[i, j, 6] / cov if has else zero
                a = tuple(max(f[i, j, k], floor_) for k in range(3)) if demodulate else (one, one, one)
                e = tuple(c[i, j, k] / a[k] for k in range(3)) if demodulate else tuple(c[i, j, k] for k in range(3))
                y = (e[0] + e[1]) + e[2]
                y2 = y * y
                assert type(y2) is T
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
                    if front and inr:
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
                            eh = [se[k] / sw for k in range(3)]
                            l1 = sl_ / sw + one
                            nn = l1 if l1 < K["n_max"] else K["n_max"]
                            alpha = one / nn
                            en = tuple(eh[k] + alpha * (e[k] - eh[k]) for k in range(3))
                            ln = nn
                            mh = sm / sw
                            mn = mh + alpha * (y2 - mh)
                            assert type(mn) is T and type(alpha) is T
                for k in range(3):
                    v = en[k] * a[k] if demodulate else en[k]
                    out[i, j, k] = np.sqrt(v) if gamma else v
                    nxt["E"][i, j, k] = en[k]
                    nxt["G"][i, j, k] = n[k]
                nxt["E"][i, j, 3] = z
                nxt["G"][i, j, 3] = cov
                nxt["L"][i, j] = ln
                M[i, j] = mn
    return out, nxt, M


# ---- the noise map -------------------------------------------------------------------------------------------------------------------------
def noise_map(state, moment, T, radius=2, m=1, sigma_depth=0.1, min_len=4.0, details=None):
    """the map's definition, vectorised: whole frames per tap -> rho [H, W] of type T, NaN where the slot is not valid"""
    T = np.dtype(T).type
    E, G, L, M = state["E"], state["G"], state["L"], np.asarray(moment)
    _is(T, E, G, L, M)
    H, W = L.shape
    inv_sz, ml = noise_constants(T, sigma_depth, min_len)
    one, zero, fl = T(1), T(0), T(2.0 ** -6)
    with np.errstate(all="ignore"):
        valid = ~np.isnan(G[..., 3])
        cov, z, n = G[..., 3], E[..., 3], G[..., 0:3]
        has = valid & (cov > zero)
        Lm = (E[..., 0] + E[..., 1]) + E[..., 2]
        vt = M - Lm * Lm
        var_t = np.where(vt > zero, vt, zero)
        _is(T, Lm, vt, var_t)
        S0, S1, S2 = np.zeros((H, W), T), np.zeros((H, W), T), np.zeros((H, W), T)
        n_taps, n_out, n_invalid, n_mixed = (np.zeros((H, W), np.int64) for _ in range(4))
        cut = np.zeros((H, W, 4), bool)
        for dj in range(-radius, radius + 1):
            for di in range(-radius, radius + 1):
                ii, jj = np.arange(H)[:, None] + di, np.arange(W)[None, :] + dj
                inside = (ii >= 0) & (ii < H) & (jj >= 0) & (jj < W)
                ok = DR._shift(valid, di, dj, False)
                eq, gq, mq = DR._shift(E, di, dj, zero), DR._shift(G, di, dj, zero), DR._shift(M, di, dj, zero)
                t_v = one - np.abs(cov - gq[..., 3])
                w_v = np.where(t_v > zero, t_v, zero)
                w = one * w_v                                         # sb = 1
                dot = (n[..., 0] * gq[..., 0] + n[..., 1] * gq[..., 1]) + n[..., 2] * gq[..., 2]
                tt = np.where(dot > zero, dot, zero)
                for _ in range(m):
                    tt = tt * tt
                zs = z + eq[..., 3]
                r = (z - eq[..., 3]) / np.where(zs > zero, zs, one)
                w_z = one / (one + (r * r) * inv_sz)
                wg = (w * tt) * w_z
                both = has & (gq[..., 3] > zero)
                w = np.where(both, wg, w)
                lq = (eq[..., 0] + eq[..., 1]) + eq[..., 2]
                t1, t2 = w * lq, w * mq
                _is(T, t_v, w_v, dot, tt, zs, r, w_z, wg, w, lq, t1, t2)
                S0 = S0 + np.where(ok, w, zero)
                S1 = S1 + np.where(ok, t1, zero)
                S2 = S2 + np.where(ok, t2, zero)
                _is(T, S0, S1, S2)
                n_taps += ok
                n_out += ~inside
                n_invalid += inside & ~ok
                n_mixed += ok & (has != (gq[..., 3] > zero))
                cut[..., 0] |= ii < 0
                cut[..., 1] |= ii >= H
                cut[..., 2] |= jj < 0
                cut[..., 3] |= jj >= W
        mu = S1 / S0
        vs = S2 / S0 - mu * mu
        var_s = np.where(vs > zero, vs, zero)
        temporal = L >= ml
        v = np.where(temporal, var_t, var_s) / L
        rho = np.sqrt(v) / np.where(Lm > fl, Lm, fl)
        _is(T, mu, vs, var_s, v, rho)
    rho = np.where(valid, rho, T(np.nan))
    _is(T, rho)
    if details is not None:
        details.update(valid=valid, has=has, temporal=temporal, vt=vt, vs=vs, n_taps=n_taps, n_out=n_out, n_invalid=n_invalid, n_mixed=n_mixed, cut=cut, S0=S0)
    return rho


def noise_map_scalar(state, moment, T, radius=2, m=1, sigma_depth=0.1, min_len=4.0):
    """the map's definition, one pixel at a time on numpy scalars of type T"""
    T = np.dtype(T).type
    E, G, L, M = state["E"], state["G"], state["L"], np.asarray(moment)
    _is(T, E, G, L, M)
    H, W = L.shape
    inv_sz, ml = noise_constants(T, sigma_depth, min_len)
    one, zero, fl = T(1), T(0), T(2.0 ** -6)
    rho = np.full((H, W), np.nan, T)
    with np.errstate(all="ignore"):
        for i in range(H):
            for j in range(W):
                gp, ep = G[i, j], E[i, j]
                if bool(np.isnan(gp[3])):
                    continue
                Lm = (ep[0] + ep[1]) + ep[2]
                ln = L[i, j]
                if bool(ln >= ml):
                    x = M[i, j] - Lm * Lm
                else:
                    S0, S1, S2 = zero, zero, zero
                    for dj in range(-radius, radius + 1):
                        for di in range(-radius, radius + 1):
                            qi, qj = i + di, j + dj
                            if not (0 <= qi < H and 0 <= qj < W) or bool(np.isnan(G[qi, qj, 3])):
                                continue
                            eq, gq = E[qi, qj], G[qi, qj]
                            t_v = one - abs(gp[3] - gq[3])
                            w = t_v if t_v > zero else zero
                            if bool(gp[3] > zero) and bool(gq[3] > zero):
                                dot = (gp[0] * gq[0] + gp[1] * gq[1]) + gp[2] * gq[2]
                                tt = dot if dot > zero else zero
                                for _ in range(m):
                                    tt = tt * tt
                                zs = ep[3] + eq[3]
                                r = (ep[3] - eq[3]) / (zs if zs > zero else one)
                                w = (w * tt) * (one / (one + (r * r) * inv_sz))
                            lq = (eq[0] + eq[1]) + eq[2]
                            assert type(w) is T and type(lq) is T
                            S0 = S0 + w
                            S1 = S1 + w * lq
                            S2 = S2 + w * M[qi, qj]
                    mu = S1 / S0
                    x = S2 / S0 - mu * mu
                var = x if x > zero else zero
                v = var / ln
                r_ = np.sqrt(v) / (Lm if Lm > fl else fl)
                assert type(r_) is T
                rho[i, j] = r_
    return rho


# ---- hand-made inputs and their census ---------------------------------------------------------------------------------------------------
def handmade_moment(state, T, seed):
    """a previous moment plane for a hand-made state: Lm^2 times a factor in [0.5, 3) per pixel -- below 1 (a moment smaller than the squared
    mean, which no history produces but a caller's buffer may hold: the variance clamps at +0) as well as above --, 0 where the slot is not
    valid"""
    T = np.dtype(T).type
    rng = np.random.default_rng(seed + 3)
    E = state["E"]
    with np.errstate(all="ignore"):
        Lm = ((E[..., 0] + E[..., 1]) + E[..., 2]).astype(np.float64)
        M = (Lm * Lm * rng.uniform(0.5, 3.0, Lm.shape)).astype(T)
    return np.where(np.isnan(state["G"][..., 3]) | ~np.isfinite(M), T(0), M).astype(T)


def handmade_sequence(H, W, T, seed, n_frames=3, rtw=None):
    """temporal_ref.handmade_sequence plus a hand-made moment plane for its previous state (whose planted history lengths 1..24 lie on both
    sides of the default min_len) -> (cams, frames, state0, moment0, cam0)"""
    cams, frames, state0, cam0 = TR.handmade_sequence(H, W, T, seed, n_frames, rtw)
    return cams, frames, state0, handmade_moment(state0, T, seed), cam0


def census(image, features, cam, T, state, moment, cam_prev, noise=None, **params):
    """which regimes one step with moments and the map of what it leaves reach, counted on the witness alone"""
    T = np.dtype(T).type
    nk = dict(NOISE_DEFAULTS)
    nk.update(noise or {})
    ds, dn = {}, {}
    _, nxt, M = step_moments(image, features, cam, T, state, moment, cam_prev, details=ds, **params)
    rho = noise_map(nxt, M, T, details=dn, **nk)
    v, temporal = dn["valid"], dn["temporal"]
    spatial = v & ~temporal
    r = nk["radius"]
    H, W = v.shape
    with np.errstate(all="ignore"):
        return dict(temporal=int((v & temporal).sum()),
                    spatial=int(spatial.sum()),
                    reset=int((ds["valid"] & ~ds["accept"] & same_mask(M, ds["y2"])).sum()),
                    accepted=int((ds["valid"] & ds["accept"]).sum()),
                    cut_top=int((spatial & dn["cut"][..., 0]).sum()), cut_bottom=int((spatial & dn["cut"][..., 1]).sum()),
                    cut_left=int((spatial & dn["cut"][..., 2]).sum()), cut_right=int((spatial & dn["cut"][..., 3]).sum()),
                    frame_smaller_than_window=int(H < 2 * r + 1 or W < 2 * r + 1) * int(spatial.sum()),
                    invalid_neighbour=int((spatial & (dn["n_invalid"] > 0)).sum()),
                    sky_covered_pair=int((spatial & (dn["n_mixed"] > 0)).sum()),
                    vt_clamped=int((v & temporal & (dn["vt"] < 0)).sum()),
                    vs_clamped=int((spatial & (dn["vs"] < 0)).sum()),
                    invalid_centre=int((~v & np.isnan(rho) & (M == 0)).sum()),
                    finite=int(np.isfinite(rho).sum()))


def same_mask(a, b):
    """elementwise: the same bits"""
    return bits(np.ascontiguousarray(a)) == bits(np.ascontiguousarray(b))
