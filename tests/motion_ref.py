"""The witness of temporal reuse over moving spheres (include/rtw_hip.h rtw_motion_table_*, rtw_first_hit_motion_*, rtw_animated_step_*): the
definition restated in numpy.  Nothing of the product is used but its camera mirror; the first hit comes from the oracle's unit call
hit_world_batch (in the oracle's current numerics mode), the frame is prepared by the denoiser's witness, the host constants, the window of
the clamp and the state's layout are the pieces of temporal_ref / temporal_clamp_ref that the motion does not change.  numpy rounds every
operation once and never fuses; the element type of every intermediate is asserted.

    centre_rays(cam, W, H, T)                           the step's own ray per pixel -> [H, W, 6] = (origin, nD)
    motion_table(flat_prev, flat, T)                    the table: one subtraction per component; NaN rows for new or changed spheres
    motion_pass(flat, cam, W, H, T, table)              the pass -> [H, W, 4] = (m, id)
    step(image, features, cam, T, motion, state, ...)   the step with motion, vectorised: plain, with moments, clamped -> (out, state, moment or None)
    step_scalar(...)                                    the same definition one pixel and one numpy scalar at a time
    handmade_motion(...) / census(...)                  a hand-made motion plane for a hand-made step and which regimes it reaches
Arrays are indexed [i, j, channel] (row, column): the library's memory is the transpose, pixel (i, j) at slot j*H + i."""
import numpy as np

import denoise_ref as DR
import rtw_oracle as O
import temporal_clamp_ref as CR
import temporal_ref as TR

_is = DR._is
bits, same_bits = DR.bits, DR.same_bits

#: the frames (W, H) of tests/test_gpu_motion.py's steps and the committed seeds of their hand-made sequences
SIZES = [(1, 1), (5, 3), (37, 23), (3, 2), (9, 33), (70, 40)]
SEEDS = {np.float32: 71, np.float64: 72}
#: the variants of the step: (moments, clamp)
VARIANTS = [(False, None), (True, None), (False, dict(radius=1, guides=False)), (True, dict(radius=1, guides=True)), (False, dict(radius=3, guides=True)),
            (True, dict(radius=3, guides=False))]


def _get(cam, k):
    return cam[k] if isinstance(cam, dict) else getattr(cam, k)


def _fields(cam, T, names):
    out = []
    for k in names:
        a = np.asarray(_get(cam, k))
        _is(T, a)
        out.append(a)
    return out


# ---- the motion pass ------------------------------------------------------------------------------------------------------------------------
def centre_rays(cam, W, H, T):
    """the step's own ray per pixel (the rtw_temporal_* block's su, tv, D, nD; the lens is ignored) -> [H, W, 6] = (cam.origin, nD)"""
    T = np.dtype(T).type
    o, llc, hor, ver = _fields(cam, T, ("origin", "lower_left_corner", "horizontal", "vertical"))
    with np.errstate(all="ignore"):
        su = (np.arange(W, dtype=np.int64).astype(T) + T(1.5)) / T(W)
        tv = ((H - np.arange(H, dtype=np.int64)).astype(T) - T(0.5)) / T(H)
        D = [((llc[k] + su * hor[k])[None, :] + (tv * ver[k])[:, None]) - o[k] for k in range(3)]
        sl = np.sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2])
        nD = [D[k] / sl for k in range(3)]
    _is(T, su, tv, sl, *D, *nD)
    rays = np.empty((H, W, 6), T)
    rays[..., 0:3] = o
    for k in range(3):
        rays[..., 3 + k] = nD[k]
    return rays


def motion_table(flat_prev, flat, T):
    """-> [n, 4] = (c_cur - c_prev, 0): one subtraction in T per component; three NaNs for a sphere with k >= n_prev or a radius that differs bitwise"""
    T = np.dtype(T).type
    n, n_prev = int(flat["n"]), int(flat_prev["n"])
    table = np.zeros((n, 4), T)
    m = min(n, n_prev)
    for c, k in enumerate(("cx", "cy", "cz")):
        cur, prev = np.asarray(flat[k], T), np.asarray(flat_prev[k], T)
        d = cur[:m] - prev[:m]
        _is(T, d)
        table[:m, c] = d
    same = bits(np.asarray(flat["r"], T)[:m]) == bits(np.asarray(flat_prev["r"], T)[:m])
    table[:m][~same, 0:3] = np.nan
    table[m:, 0:3] = np.nan
    return table


def first_hit(flat, rays, T):
    """the scan of all spheres with hit(::Sphere), tmin = 1e-4, tmax = +inf: the smallest root wins and, among equal roots, the LOWER caller's
    index -> (idx int32, t).  The oracle's loop keeps the later of two equal roots, so it runs over the scene in reversed order."""
    T = np.dtype(T).type
    n = int(flat["n"])
    rev = {k: (np.asarray(v)[::-1].copy() if isinstance(v, np.ndarray) else v) for k, v in flat.items()}
    idx, t = O.hit_world_batch(rev, rays.reshape(-1, 6), 1e-4, np.inf, T)
    return np.where(idx >= 0, n - 1 - idx, -1).astype(np.int32), t


def motion_pass(flat, cam, W, H, T, table=None):
    """the pass -> [H, W, 4]: (table[k].xyz, T(k)) on a hit of sphere k, (0, 0, 0, -1) on a miss; table None: m = 0"""
    T = np.dtype(T).type
    idx, _ = first_hit(flat, centre_rays(cam, W, H, T), T)
    idx = idx.reshape(H, W)
    out = np.zeros((H, W, 4), T)
    hit = idx >= 0
    if table is not None:
        _is(T, table)
        out[hit, 0:3] = table[idx[hit], 0:3]
    out[..., 3] = idx.astype(T)
    return out


# ---- the step -------------------------------------------------------------------------------------------------------------------------------
def step(image, features, cam, T, motion=None, state=None, cam_prev=None, moment=None, moments=None, clamp=None, m=1, sigma_depth=0.1, min_weight=0.25,
         history_max=16.0, demodulate=True, gamma=1, details=None):
    """the definition, vectorised -> (out [H, W, 3], the next state, the next moment plane -- None without moments).  `motion` [H, W, 4] is
    there exactly when the previous state is; `clamp` None: the plain step, else temporal_clamp_ref's dict; `moments` defaults to whether a
    moment plane is given.  The ONE line that differs from temporal_ref.step / temporal_clamp_ref.step_clamped is the one that forms d."""
    T = np.dtype(T).type
    ck = CR._clamp(clamp) if clamp is not None else None
    if moments is None:
        moments = moment is not None
    assert (state is None) == (cam_prev is None) == (motion is None) and (moment is None or (moments and state is not None)) and not (moments and state is not None and moment is None)
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
            Ep, Gp, Lp = state["E"], state["G"], state["L"]
            Mp = np.asarray(moment) if moments else np.zeros((H, W), T)
            mv = np.asarray(motion)
            assert mv.shape == (H, W, 4)
            _is(T, Ep, Gp, Lp, Mp, mv)
            if ck is not None:
                lo, hi = CR.window_bounds(valid, has, e, n, z, cov, T, ck["radius"], ck["guides"], ck["sigma"], m, sigma_depth)
                ks, ls = CR.clamp_constants(T, ck["sigma"], ck["len_scale"])
            o, llc, hor, ver = _fields(cam, T, ("origin", "lower_left_corner", "horizontal", "vertical"))
            po, pw, ph, pv = _fields(cam_prev, T, ("origin", "w", "horizontal", "vertical"))
            su = (np.arange(W, dtype=np.int64).astype(T) + T(1.5)) / T(W)
            tv = ((H - np.arange(H, dtype=np.int64)).astype(T) - T(0.5)) / T(H)
            D = [((llc[k] + su * hor[k])[None, :] + (tv * ver[k])[:, None]) - o[k] for k in range(3)]
            sl = np.sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2])
            nD = [D[k] / sl for k in range(3)]
            # the point to reproject, moved back to where the surface was one frame ago, relative to the previous origin
            d = [np.where(has, ((o[k] + z * nD[k]) - mv[..., k]) - po[k], nD[k]) for k in range(3)]
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
            hc, lc = eh, lh
            if ck is not None:
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
                details.update(front=front, inr=inr, x0=x0, y0=y0, x=x, y=yy)
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
        details.update(valid=valid, has=has, accept=accept)
    return out, nxt, M


def step_scalar(image, features, cam, T, motion=None, state=None, cam_prev=None, moment=None, moments=None, clamp=None, m=1, sigma_depth=0.1, min_weight=0.25,
                history_max=16.0, demodulate=True, gamma=1):
    """the same definition, one pixel at a time on numpy scalars of type T (for small frames)"""
    T = np.dtype(T).type
    ck = CR._clamp(clamp) if clamp is not None else None
    if moments is None:
        moments = moment is not None
    assert (state is None) == (cam_prev is None) == (motion is None)
    c, f = np.asarray(image), np.asarray(features)
    _is(T, c, f)
    H, W = c.shape[:2]
    K = TR.host_constants(cam_prev, T, sigma_depth, min_weight, history_max)
    if ck is not None:
        ks, ls = CR.clamp_constants(T, ck["sigma"], ck["len_scale"])
        R = ck["radius"]
    one, zero, floor_ = T(1), T(0), T(2.0 ** -6)
    out = np.full((H, W, 3), np.nan, T)
    nxt = TR.empty_state(H, W, T)
    nxt["G"][..., 3] = np.nan
    M = np.zeros((H, W), T)
    dot3 = lambda u, v: (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]

    def prep(i, j):
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
        o, llc, hor, ver = _fields(cam, T, ("origin", "lower_left_corner", "horizontal", "vertical"))
        po, pw, ph, pv = _fields(cam_prev, T, ("origin", "w", "horizontal", "vertical"))
        Ep, Gp, Lp = state["E"], state["G"], state["L"]
        Mp = np.asarray(moment) if moments else np.zeros((H, W), T)
        mv = np.asarray(motion)
        _is(T, mv)
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
                    d = [((o[k] + z * nD[k]) - mv[i, j, k]) - po[k] for k in range(3)] if has else nD
                    dw = dot3(d, pw)
                    front = bool(dw < zero)
                    lam = K["Kw"] / dw
                    s = (lam * dot3(d, ph) - K["Qh"]) * K["ih"]
                    t = (lam * dot3(d, pv) - K["Qv"]) * K["iv"]
                    x = s * T(W) - T(1.5)
                    yy = (T(H) - T(0.5)) - t * T(H)
                    inr = bool(x > T(-1) and x < T(W) and yy > T(-1) and yy < T(H))
                    assert all(type(v) is T for v in (su, tv, sl, dw, lam, s, t, x, yy, *d))
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
                            lh = sl_ / sw
                            hc = eh
                            if ck is not None:
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
                                            S0 = S0 + w
                                            for k in range(3):
                                                S1[k] = S1[k] + w * eq[k]
                                                S2[k] = S2[k] + w * (eq[k] * eq[k])
                                        else:
                                            S0 = S0 + one
                                            for k in range(3):
                                                S1[k] = S1[k] + eq[k]
                                                S2[k] = S2[k] + eq[k] * eq[k]
                                hc, moved = [None] * 3, False
                                for k in range(3):
                                    mu = S1[k] / S0
                                    vt = S2[k] / S0 - mu * mu
                                    sd = np.sqrt(vt if vt > zero else zero)
                                    lo, hi = mu - ks * sd, mu + ks * sd
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


# ---- a hand-made motion plane and its census ------------------------------------------------------------------------------------------------
#: displacements in pixels (columns, rows) at the pixel's own depth that a hand-made plane is built from: the first six at random, all of them to plant regimes
SHIFTS = [(1, 0), (-1, 0), (0, 1), (0, -1), (2, 1), (-2, -1), (3, 0), (-3, 0), (0, 2), (0, -2), (4, 1), (-4, -1), (1, 3), (-1, -3), (6, 0), (-6, 0)]
N_RANDOM_SHIFTS = 6
#: ... and the finer, wider grid that is searched only when a regime could not be planted from SHIFTS (the smallest frames)
MORE_SHIFTS = [(dx / 2, dy / 2) for dx in range(-10, 11) for dy in range(-6, 7) if (dx, dy) != (0, 0)]


def _shift_plane(image, features, cam, T, shift, demodulate=True):
    """the plane that moves every covered pixel by `shift` pixels at its own depth: m = z * (dx * hor / W + dy * ver / H), in binary64, rounded to T
    (focus_dist is 1 in the hand-made cameras, so hor / W is one pixel at distance 1); uncovered pixels get 0"""
    T = np.dtype(T).type
    _, has, _, _, z, _, _ = DR.prepare(image, features, T, demodulate)
    H, W = has.shape
    hor, ver = (np.asarray(_get(cam, k)).astype(np.float64) for k in ("horizontal", "vertical"))
    step_ = shift[0] * hor / W + shift[1] * ver / H
    plane = np.zeros((H, W, 4), T)
    with np.errstate(all="ignore"):
        plane[..., 0:3] = np.where(has[..., None], z.astype(np.float64)[..., None] * step_, 0.0).astype(T)
    return plane


def handmade_motion(image, features, cam, T, state, cam_prev, seed, **params):
    """A hand-made motion plane for one hand-made step.  Every covered pixel gets one of the first N_RANDOM_SHIFTS displacements or none,
    drawn by `seed`; the fourth element holds arbitrary values, NaN among them (it has no effect on the step); then four regimes are planted,
    each at the first pixel in column-major order that admits it and has not been used: a pixel the plain step resets and some shift
    accepts; one the plain step accepts and some shift resets; an accepted pixel whose first tap (x0, y0) moves; a pixel the plain step
    accepts that gets a non-finite slot (NaN in one component, in all three, +inf: one each where three such pixels exist).  A frame that
    does not admit a regime simply lacks it: census() says what is there."""
    T = np.dtype(T).type
    H, W = np.asarray(image).shape[:2]
    rng = np.random.default_rng(seed + 11)
    zero_plane = np.zeros((H, W, 4), T)
    d0 = {}
    step(image, features, cam, T, zero_plane, state, cam_prev, details=d0, **params)
    planes, det = [], []

    def evaluate(shifts):
        for sh in shifts:
            p = _shift_plane(image, features, cam, T, sh, params.get("demodulate", True))
            dd = {}
            step(image, features, cam, T, p, state, cam_prev, details=dd, **params)
            planes.append(p)
            det.append(dd)
    evaluate(SHIFTS)

    def evaluate_targets():
        """the last resort of the smallest frames: planes that send every covered pixel exactly onto the centre of ONE pixel q of the previous
        view, at the depth the previous state holds there (binary64, rounded to T) -- one plane per valid covered slot q"""
        rays, rays_p = centre_rays(cam, W, H, T).astype(np.float64), centre_rays(cam_prev, W, H, T).astype(np.float64)
        _, has_, _, _, z_, _, _ = DR.prepare(image, features, T, params.get("demodulate", True))
        Pw = rays[..., 0:3] + z_.astype(np.float64)[..., None] * rays[..., 3:6]
        for qi in range(H):
            for qj in range(W):
                if not state["G"][qi, qj, 3] > 0:
                    continue
                Pq = rays_p[qi, qj, 0:3] + np.float64(state["E"][qi, qj, 3]) * rays_p[qi, qj, 3:6]
                p = np.zeros((H, W, 4), T)
                with np.errstate(all="ignore"):
                    p[..., 0:3] = np.where(has_[..., None], Pw - Pq, 0.0).astype(T)
                dd = {}
                step(image, features, cam, T, p, state, cam_prev, details=dd, **params)
                planes.append(p)
                det.append(dd)
    pick = rng.integers(-1, N_RANDOM_SHIFTS, size=(H, W))
    plane = zero_plane.copy()
    for k in range(N_RANDOM_SHIFTS):
        plane[pick == k] = planes[k][pick == k]
    plane[..., 3] = rng.integers(-1, 500, size=(H, W)).astype(T)
    plane[..., 3][rng.random((H, W)) < 0.1] = np.nan
    plane[H - 1, W - 1, 3] = np.nan
    v, has, acc0 = d0["valid"], d0["has"], d0["accept"]
    sky = ~has & (rng.random((H, W)) < 0.5)                         # (a pixel that is not covered ignores its slot, whatever it holds)
    plane[sky, 0:3] = rng.uniform(-2, 2, (int(sky.sum()), 3)).astype(T)
    used = np.zeros((H, W), bool)
    order = [(i, j) for j in range(W) for i in range(H)]

    def plant(cond_of_shift):
        for first in (0, len(SHIFTS), len(SHIFTS) + len(MORE_SHIFTS)):
            if first == len(SHIFTS) and len(det) == first:
                evaluate(MORE_SHIFTS)
            if first > len(SHIFTS) and len(det) == first:
                if H * W > 64:
                    return
                evaluate_targets()
            for (i, j) in order:
                if used[i, j] or not (v[i, j] and has[i, j]):
                    continue
                for k in range(first, len(det)):
                    if cond_of_shift(det[k], i, j):
                        plane[i, j, 0:3] = planes[k][i, j, 0:3]
                        used[i, j] = True
                        return
    plant(lambda dd, i, j: not acc0[i, j] and dd["accept"][i, j])
    plant(lambda dd, i, j: acc0[i, j] and not dd["accept"][i, j])
    plant(lambda dd, i, j: acc0[i, j] and dd["accept"][i, j] and (dd["x0"][i, j] != d0["x0"][i, j] or dd["y0"][i, j] != d0["y0"][i, j]))
    bad = [(np.nan, 0.25, 0.0), (np.nan, np.nan, np.nan), (0.0, np.inf, 0.0)]
    for (i, j) in order:
        if bad and not used[i, j] and v[i, j] and has[i, j] and acc0[i, j]:
            plane[i, j, 0:3] = np.array(bad.pop(0), T)
            used[i, j] = True
    return plane


def census(image, features, cam, T, motion, state, cam_prev, **params):
    """which regimes of the motion one step reaches, counted on the witness alone: the step with `motion` against the step with a plane of zeros"""
    T = np.dtype(T).type
    d0, d1 = {}, {}
    step(image, features, cam, T, np.zeros_like(motion), state, cam_prev, details=d0, **params)
    step(image, features, cam, T, motion, state, cam_prev, details=d1, **params)
    v, has = d1["valid"], d1["has"]
    fin = np.isfinite(motion[..., 0:3]).all(axis=-1)
    a0, a1 = d0["accept"], d1["accept"]
    moved_tap = (d0["x0"] != d1["x0"]) | (d0["y0"] != d1["y0"])
    return dict(moved_accepted=int((v & a0 & a1 & fin & moved_tap).sum()),
                nan_reset=int((v & has & a0 & ~a1 & ~fin).sum()),
                gained=int((v & ~a0 & a1).sum()),
                lost=int((v & a0 & ~a1 & fin).sum()),
                sky_with_motion=int((v & ~has & (motion[..., 0:3] != 0).any(axis=-1)).sum()),
                accepted=int((v & a1).sum()))


def handmade_steps(H, W, T, seed, rtw=None):
    """the hand-made steps of one frame size: temporal_noise_ref's sequence (cameras, frames, a previous state with its moment plane) chained by
    the PLAIN witness step with moments, each step with its own hand-made motion plane -> a list of dicts image, features, cam, cam_prev,
    state, moment, motion (the inputs of step k)"""
    import temporal_noise_ref as NR
    cams, frames, state, moment, cam_prev = NR.handmade_sequence(H, W, T, seed, rtw=rtw)
    out = []
    for k, (cam, (image, feat)) in enumerate(zip(cams, frames)):
        motion = handmade_motion(image, feat, cam, T, state, cam_prev, seed + 100 * k)
        out.append(dict(image=image, features=feat, cam=cam, cam_prev=cam_prev, state=state, moment=moment, motion=motion))
        _, state, moment = step(image, feat, cam, T, motion, state, cam_prev, moment)
        cam_prev = cam
    return out
