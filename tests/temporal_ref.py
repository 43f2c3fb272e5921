"""The witness of the temporal reprojection (include/rtw_hip.h rtw_temporal_*): the definition restated in numpy from nothing of the product
but its camera mirror (a plain record of arrays).  The frame is prepared by the denoiser's witness (denoise_ref.prepare); everything else is
restated here.  Every intermediate has the element type T (asserted); numpy rounds every operation once and never fuses.

    step(image, features, cam, T, state, cam_prev, ...)          vectorised: whole frames per tap -> (out, next state)
    step_scalar(image, features, cam, T, state, cam_prev, ...)   the same definition one pixel and one numpy scalar at a time
    host_constants(cam_prev, T, ...)                             what the library's host computes in binary64 and rounds to T
    pack_state(state, T) / unpack_state(flat, H, W)              a state <-> the library's memory (the public layout of the header)
    handmade_sequence(H, W, T, seed, n_frames)                   cameras, hand-made frames and a hand-made previous state
    census(...)                                                  which branches of the definition a step reaches, counted on the witness alone
A state is a dict E [H, W, 4] = (e', z), G [H, W, 4] = (n, cov; NaN: not valid), L [H, W] = len.
Arrays are indexed [i, j, channel] (row, column): the library's memory is the transpose, pixel (i, j) at j*H + i."""
import numpy as np

import denoise_ref as DR

DEFAULTS = dict(m=1, sigma_depth=0.1, min_weight=0.25, history_max=16.0, demodulate=True, gamma=1)
_is = DR._is
bits, same_bits = DR.bits, DR.same_bits

#: the frames (W, H) of tests/test_gpu_temporal.py and the committed seeds of their hand-made sequences
SIZES = [(1, 1), (5, 3), (37, 23), (70, 41)]
SEEDS = {np.float32: 41, np.float64: 42}


def _dot64(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def host_constants(cam_prev, T, sigma_depth, min_weight, history_max):
    """what the host computes in binary64 -> dict of T scalars: Kw, Qh, Qv, ih, iv (None camera: absent), inv_sz, w_min, n_max"""
    T = np.dtype(T).type
    c = {}
    with np.errstate(all="ignore"):
        if cam_prev is not None:
            o, llc, hor, ver, w = (np.asarray(getattr(cam_prev, k)).astype(np.float64) for k in ("origin", "lower_left_corner", "horizontal", "vertical", "w"))
            q = llc - o
            c.update(Kw=T(_dot64(q, w)), Qh=T(_dot64(q, hor)), Qv=T(_dot64(q, ver)), ih=T(np.float64(1.0) / _dot64(hor, hor)), iv=T(np.float64(1.0) / _dot64(ver, ver)))
        c.update(inv_sz=T(np.float64(1.0) / np.float64(float(sigma_depth) * float(sigma_depth))), w_min=T(np.float64(min_weight)), n_max=T(np.float64(history_max)))
    return c


def _cam_fields(cam, T, names):
    out = []
    for k in names:
        a = np.asarray(getattr(cam, k))
        _is(T, a)
        out.append(a)
    return out


def empty_state(H, W, T):
    return dict(E=np.zeros((H, W, 4), T), G=np.zeros((H, W, 4), T), L=np.zeros((H, W), T))


def state_elems(H, W, T):
    """elements of T in a packed state: 9*W*H of them, rounded up to 16 bytes"""
    eb = np.dtype(T).itemsize
    return ((9 * W * H * eb + 15) // 16 * 16) // eb


def pack_state(state, T):
    """-> the flat array the library reads: plane E, plane G, plane L, pixel (i, j) at slot j*H + i; zero padding up to 16 bytes"""
    H, W = state["L"].shape
    flat = np.zeros(state_elems(H, W, T), T)
    n = W * H
    flat[:4 * n] = np.swapaxes(state["E"], 0, 1).reshape(-1)
    flat[4 * n:8 * n] = np.swapaxes(state["G"], 0, 1).reshape(-1)
    flat[8 * n:9 * n] = np.swapaxes(state["L"], 0, 1).reshape(-1)
    return flat


def unpack_state(flat, H, W):
    n = W * H
    return dict(E=np.swapaxes(flat[:4 * n].reshape(W, H, 4), 0, 1).copy(), G=np.swapaxes(flat[4 * n:8 * n].reshape(W, H, 4), 0, 1).copy(),
                L=np.swapaxes(flat[8 * n:9 * n].reshape(W, H), 0, 1).copy())


def step(image, features, cam, T, state=None, cam_prev=None, m=1, sigma_depth=0.1, min_weight=0.25, history_max=16.0, demodulate=True, gamma=1, details=None):
    """the definition, vectorised -> (out [H, W, 3] of type T, NaN where the pixel is not valid; the next state).  `details`: a dict that
    receives the intermediates census() counts on"""
    T = np.dtype(T).type
    assert (state is None) == (cam_prev is None)
    valid, has, e, n, z, cov, a = DR.prepare(image, features, T, demodulate)
    H, W = valid.shape
    K = host_constants(cam_prev, T, sigma_depth, min_weight, history_max)
    one, zero = T(1), T(0)
    with np.errstate(all="ignore"):
        if state is None:
            accept = np.zeros((H, W), bool)
            en, ln = e.copy(), np.ones((H, W), T)
        else:
            Ep, Gp, Lp = state["E"], state["G"], state["L"]
            _is(T, Ep, Gp, Lp)
            o, llc, hor, ver = _cam_fields(cam, T, ("origin", "lower_left_corner", "horizontal", "vertical"))
            po, pw, ph, pv = _cam_fields(cam_prev, T, ("origin", "w", "horizontal", "vertical"))
            # the pixel's own ray in the current camera
            su = (np.arange(W, dtype=np.int64).astype(T) + T(1.5)) / T(W)
            tv = ((H - np.arange(H, dtype=np.int64)).astype(T) - T(0.5)) / T(H)
            D = [((llc[k] + su * hor[k])[None, :] + (tv * ver[k])[:, None]) - o[k] for k in range(3)]
            l2 = (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]
            sl = np.sqrt(l2)
            nD = [D[k] / sl for k in range(3)]
            _is(T, su, tv, l2, sl, *D, *nD)
            # the point to reproject, relative to the previous origin
            d = [np.where(has, (o[k] + z * nD[k]) - po[k], nD[k]) for k in range(3)]
            dot3 = lambda v: (d[0] * v[0] + d[1] * v[1]) + d[2] * v[2]
            dw = dot3(pw)
            front = dw < zero
            lam = K["Kw"] / dw
            s = (lam * dot3(ph) - K["Qh"]) * K["ih"]
            t = (lam * dot3(pv) - K["Qv"]) * K["iv"]
            x = s * T(W) - T(1.5)
            y = (T(H) - T(0.5)) - t * T(H)
            inr = (x > T(-1)) & (x < T(W)) & (y > T(-1)) & (y < T(H))
            xs, ys = np.where(inr, x, zero), np.where(inr, y, zero)
            xf, yf = np.floor(xs), np.floor(ys)
            x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
            fx, fy = xs - xf, ys - yf
            zexp = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            _is(T, *d, dw, lam, s, t, x, y, xs, ys, xf, yf, fx, fy, zexp)
            valid_q = ~np.isnan(Gp[..., 3])
            sum_w, sum_l, sum_e = np.zeros((H, W), T), np.zeros((H, W), T), np.zeros((H, W, 3), T)
            n_inside, n_visited, n_skipped_invalid, n_wv0, n_sky_taps = (np.zeros((H, W), np.int64) for _ in range(5))
            for b in (0, 1):
                kx = fx if b else one - fx
                for c in (0, 1):
                    ky = fy if c else one - fy
                    sb = ky * kx
                    qi, qj = y0 + c, x0 + b
                    inside = (qi >= 0) & (qi < H) & (qj >= 0) & (qj < W)
                    gi, gj = np.clip(qi, 0, H - 1), np.clip(qj, 0, W - 1)
                    ok = inside & valid_q[gi, gj]
                    eq, gq, lq = Ep[gi, gj], Gp[gi, gj], Lp[gi, gj]
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
                    _is(T, kx, ky, sb, t_v, w_v, w, dot, tt, zs, r, w_z, wg)
                    w = np.where(has & (gq[..., 3] > zero), wg, w)
                    term, lterm = w[..., None] * eq[..., 0:3], w * lq
                    _is(T, w, term, lterm)
                    # a skipped tap adds nothing: the sums are never -0 (they start at +0), so adding +0 is skipping
                    sum_w = sum_w + np.where(ok, w, zero)
                    sum_e = sum_e + np.where(ok[..., None], term, zero)
                    sum_l = sum_l + np.where(ok, lterm, zero)
                    _is(T, sum_w, sum_e, sum_l)
                    n_inside += inside
                    n_visited += ok
                    n_skipped_invalid += inside & ~valid_q[gi, gj]
                    n_wv0 += ok & (w_v == zero) & ((cov > zero) != (gq[..., 3] > zero))
                    n_sky_taps += ok & (gq[..., 3] == zero) & (w > zero)
            accept = front & inr & (sum_w >= K["w_min"])
            eh = sum_e / sum_w[..., None]
            lh = sum_l / sum_w
            l1 = lh + one
            nn = np.where(l1 < K["n_max"], l1, K["n_max"])
            alpha = one / nn
            eb = eh + alpha[..., None] * (e - eh)
            _is(T, eh, lh, l1, nn, alpha, eb)
            en = np.where(accept[..., None], eb, e)
            ln = np.where(accept, nn, one)
            if details is not None:
                details.update(front=front, inr=inr, sum_w=sum_w, n_inside=n_inside, n_visited=n_visited, n_skipped_invalid=n_skipped_invalid, n_wv0=n_wv0, n_sky_taps=n_sky_taps,
                               saturated=accept & ~(l1 < K["n_max"]), x=x, y=y, lh=lh, eh=eh, alpha=alpha)
        out = en * a if demodulate else en.copy()
        if gamma:
            out = np.sqrt(out)
    _is(T, en, ln, out)
    out[~valid] = np.nan
    nxt = empty_state(H, W, T)
    nxt["E"][..., 0:3] = np.where(valid[..., None], en, zero)
    nxt["E"][..., 3] = z
    nxt["G"][..., 0:3] = n
    nxt["G"][..., 3] = np.where(valid, cov, T(np.nan))
    nxt["L"][...] = np.where(valid, ln, zero)
    if details is not None:
        details.update(valid=valid, has=has, accept=accept, e=e, a=a)
    return out, nxt


def step_scalar(image, features, cam, T, state=None, cam_prev=None, m=1, sigma_depth=0.1, min_weight=0.25, history_max=16.0, demodulate=True, gamma=1):
    """the definition, one pixel at a time on numpy scalars of type T (for tiny frames)"""
    T = np.dtype(T).type
    assert (state is None) == (cam_prev is None)
    c, f = np.asarray(image), np.asarray(features)
    _is(T, c, f)
    H, W = c.shape[:2]
    K = host_constants(cam_prev, T, sigma_depth, min_weight, history_max)
    one, zero, floor_ = T(1), T(0), T(2.0 ** -6)
    out = np.full((H, W, 3), np.nan, T)
    nxt = empty_state(H, W, T)
    nxt["G"][..., 3] = np.nan
    if state is not None:
        o, llc, hor, ver = _cam_fields(cam, T, ("origin", "lower_left_corner", "horizontal", "vertical"))
        po, pw, ph, pv = _cam_fields(cam_prev, T, ("origin", "w", "horizontal", "vertical"))
        Ep, Gp, Lp = state["E"], state["G"], state["L"]
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
                en, ln = e, one
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
                    y = (T(H) - T(0.5)) - t * T(H)
                    inr = bool(x > T(-1) and x < T(W) and y > T(-1) and y < T(H))
                    assert all(type(v) is T for v in (su, tv, sl, dw, lam, s, t, x, y))
                    if front and inr:                           # (otherwise the pixel resets whatever the taps hold)
                        xf, yf = np.floor(x), np.floor(y)
                        x0, y0 = int(xf), int(yf)
                        fx, fy = x - xf, y - yf
                        zexp = np.sqrt(dot3(d, d))
                        sw, sl_, se = zero, zero, [zero, zero, zero]
                        for b in (0, 1):
                            kx = fx if b else one - fx
                            for cc in (0, 1):
                                ky = fy if cc else one - fy
                                sb = ky * kx
                                qi, qj = y0 + cc, x0 + b
                                if not (0 <= qi < H and 0 <= qj < W) or bool(np.isnan(Gp[qi, qj, 3])):
                                    continue
                                eq, gq, lq = Ep[qi, qj], Gp[qi, qj], Lp[qi, qj]
                                t_v = one - abs(cov - gq[3])
                                w_v = t_v if t_v > zero else zero
                                w = sb * w_v
                                if has and bool(gq[3] > zero):
                                    dot = (n[0] * gq[0] + n[1] * gq[1]) + n[2] * gq[2]
                                    tt = dot if dot > zero else zero
                                    for _ in range(m):
                                        tt = tt * tt
                                    zs = zexp + eq[3]
                                    r = (zexp - eq[3]) / (zs if zs > zero else one)
                                    w_z = one / (one + (r * r) * K["inv_sz"])
                                    w = (w * tt) * w_z
                                assert type(w) is T and type(sb) is T
                                sw = sw + w
                                sl_ = sl_ + w * lq
                                for k in range(3):
                                    se[k] = se[k] + w * eq[k]
                        if bool(sw >= K["w_min"]):
                            eh = [se[k] / sw for k in range(3)]
                            l1 = sl_ / sw + one
                            nn = l1 if l1 < K["n_max"] else K["n_max"]
                            alpha = one / nn
                            en = tuple(eh[k] + alpha * (e[k] - eh[k]) for k in range(3))
                            ln = nn
                            assert type(alpha) is T and all(type(v) is T for v in en)
                for k in range(3):
                    v = en[k] * a[k] if demodulate else en[k]
                    out[i, j, k] = np.sqrt(v) if gamma else v
                    nxt["E"][i, j, k] = en[k]
                    nxt["G"][i, j, k] = n[k]
                nxt["E"][i, j, 3] = z
                nxt["G"][i, j, 3] = cov
                nxt["L"][i, j] = ln
    return out, nxt


def geometry_bound(cam, W, H, T, z_min):
    """How far, in pixels, the reprojected position (x, y) of a pixel may lie from its exact value when both cameras have `cam`'s orientation
    and viewport and every covered pixel's depth is at least z_min -> (bound_x, bound_y).  First order in the unit roundoff u of T (the
    neglected terms are u times smaller), every constant rounded up.  With h = |hor|, v = |ver|, f = |q.w| the focus distance,
    c = f / sqrt(f^2 + (h/2)^2 + (v/2)^2) the least cosine between a pixel's ray and the axis, M = max_k (|o_k| + |llc_k| + 1.05 (|hor_k| + |ver_k|))
    the largest partial sum of D, O = max_k |o_k| / z_min, and eps the camera's own departure from orthogonality (the largest cosine between
    two of hor, ver, w, measured in binary64):
        D per component    su and tv carry one quotient, each product one rounding, three additions of partial sums <= M:  6 u M, so |dD| <= sqrt(3) 6 u M
        nD = D / |D|       l2 3 u (sums of squares), sqrt 1.5 u + u, the quotient u: 3.5 u relative; |D| >= f
        d  (covered)       z*nD, + o, - o_prev, and the depth's own rounding: (4 + O) u z per component; (sky) d = nD
        eta = |dd| / |d|   <= (sqrt(3) (6 M / f + 4 + O) + 3.5) u
        a dot product      three products, two sums: 3 u |d| |b| on top of eta |d| |b|
        lam = Kw / dw      u (Kw) + u (quotient) + (3 u + eta) / c          (|dw| >= c |d|)
        p = lam * dh       (3 u + eta) f h / c  +  0.55 h^2 (3 u + (3 u + eta) / c)      (|lam dh| = |s - 1/2| h^2 <= 0.55 h^2)
        s = (p - Qh) * ih  dp / h^2 + 1.55 u (Qh's rounding, the difference) + 2.1 u (ih's rounding, the product)
        orthogonality      eps (0.55 (h + v) / f + 1.05 v / h)             (lam departs from 1, ver.hor from 0)
        x = s*W - 1.5      W ds + 2.1 u W                                   (the product, the difference)
    and the same for y with h and v exchanged."""
    u = float(np.finfo(T).eps) / 2
    o, llc, hor, ver, w = (np.asarray(getattr(cam, k)).astype(np.float64) for k in ("origin", "lower_left_corner", "horizontal", "vertical", "w"))
    h, v = float(np.linalg.norm(hor)), float(np.linalg.norm(ver))
    f = abs(float(_dot64(llc - o, w)))
    c = f / np.sqrt(f * f + h * h / 4 + v * v / 4)
    M = float(np.max(np.abs(o) + np.abs(llc) + 1.05 * (np.abs(hor) + np.abs(ver))))
    O = float(np.max(np.abs(o))) / float(z_min)
    eps = max(abs(float(_dot64(hor, ver))) / (h * v), abs(float(_dot64(hor, w))) / (h * np.linalg.norm(w)), abs(float(_dot64(ver, w))) / (v * np.linalg.norm(w)))
    eta = (np.sqrt(3.0) * (6 * M / f + 4 + O) + 3.5) * u

    def axis(n, a, b):               # a: the axis' own viewport vector length, b: the other's
        dp = (3 * u + eta) * f * a / c + 0.55 * a * a * (3 * u + (3 * u + eta) / c)
        ds = dp / (a * a) + 3.65 * u + eps * (0.55 * (a + b) / f + 1.05 * b / a)
        return n * ds + 2.1 * u * n

    return axis(W, h, v), axis(H, v, h)


def same_state(got, ref):
    """two states agree on the bits (NaN coverage as a set)"""
    return all(same_bits(got[k], ref[k]) for k in ("E", "G", "L"))


def make_camera(rtw, T, lookfrom, lookat, W, H, vfov=90):
    """a pinhole camera of the package's own camera mirror whose viewport has the frame's aspect ratio"""
    return rtw.default_camera(lookfrom=lookfrom, lookat=lookat, vup=(0, 1, 0), vfov=vfov, aspect_ratio=W / H, aperture=0, focus_dist=1, elem_type=T)


#: the camera path of the hand-made sequences: a translation with a pan of a few pixels, so that an edge band leaves the previous frame
PATH = [((0.0, 0.0, 0.0), (0.0, 0.0, -1.0)), ((0.15, 0.05, 0.0), (0.4, -0.1, -1.0)), ((0.3, 0.1, -0.05), (0.75, -0.15, -1.0))]


def handmade_frame(H, W, T, seed):
    """denoise_ref.handmade's frame with two planted regions, so that histories are accepted as well as rejected: the columns [0, W/3) are a
    surface at distance 8 with one normal and full coverage, the columns [W/3, W/2) are sky (coverage 0); the rest keeps every regime of
    handmade (coverage 0 / fractional / 1, tiny albedo, z <= 0 -- a point behind the camera --, pixels that are not finite)."""
    T = np.dtype(T).type
    image, feat = DR.handmade(H, W, T, seed)
    a, b = W // 3, W // 2
    feat[:, :a, 3:8] = np.array([0.0, 0.6, 0.8, 8.0, 1.0], T)
    feat[:, a:b, 3:8] = T(0)
    for arr in (image, feat):                               # (the planted regions are finite; the rest keeps handmade's own non-finite pixels)
        arr[:, :b] = np.where(np.isfinite(arr[:, :b]), arr[:, :b], T(0.5))
    if H * W >= 12:
        image[0, W - 1, 1] = np.nan                         # one on the border of the random region, one inside the surface
        feat[H - 1, min(1, W - 1), 7] = np.inf
    return image, feat


def handmade_sequence(H, W, T, seed, n_frames=3, rtw=None):
    """-> (cams, frames, state0, cam0): `n_frames` cameras (<= 3) along PATH built with the package's own camera mirror, a hand-made (image,
    features) per camera, and a hand-made previous state for the first of them, as seen from cam0 = cams[0] panned back by a pixel or two:
    the state a first-frame step leaves on another hand-made frame, with history lengths 1..24 planted (so that len saturates at the
    default history_max) and a few slots made not valid."""
    if rtw is None:
        import rtw_amd as rtw
    T = np.dtype(T).type
    assert 1 <= n_frames <= len(PATH)
    cams = [make_camera(rtw, T, *PATH[k], W, H) for k in range(n_frames)]
    frames = [handmade_frame(H, W, T, seed + 10 * k) for k in range(n_frames)]
    cam0 = make_camera(rtw, T, (-0.1, -0.05, 0.02), (-0.3, 0.1, -1.0), W, H)
    rng = np.random.default_rng(seed + 5)
    _, state0 = step(*handmade_frame(H, W, T, seed + 7), cam0, T)
    ok = ~np.isnan(state0["G"][..., 3])
    state0["L"] = np.where(ok, rng.integers(1, 25, size=(H, W)), 0).astype(T)
    if H * W >= 12:
        for _ in range(3):
            i, j = int(rng.integers(H)), int(rng.integers(W))
            state0["E"][i, j] = 0
            state0["G"][i, j] = (0, 0, 0, np.nan)
            state0["L"][i, j] = 0
    return cams, frames, state0, cam0


def census(image, features, cam, T, state, cam_prev, **params):
    """which branches of the definition one step reaches, counted on the witness alone (valid pixels, but for the last entry)"""
    T = np.dtype(T).type
    d = {}
    step(image, features, cam, T, state, cam_prev, details=d, **params)
    v, acc = d["valid"], d["accept"]
    w_min = T(np.float64(params.get("min_weight", DEFAULTS["min_weight"])))
    with np.errstate(all="ignore"):
        return dict(accepted=int((v & acc).sum()),
                    reset_not_front=int((v & ~d["front"]).sum()),
                    reset_not_inr=int((v & d["front"] & ~d["inr"]).sum()),
                    reset_low_weight=int((v & d["front"] & d["inr"] & ~(d["sum_w"] >= w_min) & (d["n_visited"] > 0)).sum()),
                    fewer_than_4_inside=int((v & d["inr"] & (d["n_inside"] < 4)).sum()),
                    tap_not_valid=int((v & d["inr"] & (d["n_skipped_invalid"] > 0)).sum()),
                    sky_from_sky=int((v & acc & ~d["has"] & (d["n_sky_taps"] > 0)).sum()),        # (a visited tap with cov_q = 0 and a positive weight)
                    sky_hit_mismatch=int((v & d["inr"] & (d["n_wv0"] > 0)).sum()),
                    len_saturated=int((v & d["saturated"]).sum()),
                    non_finite=int((~v).sum()))
