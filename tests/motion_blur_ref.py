"""The witness of the motion-blur stage (include/rtw_hip.h rtw_velocity_blur_*): the definition restated in numpy, twice -- vectorised over the
frame and one pixel at a time on numpy scalars.  Nothing of the product is used; the frame is prepared by the denoiser's witness, the host
constants are temporal_ref's and the pixel's own ray is motion_ref's.  numpy rounds every operation once and never fuses; the element type
of every intermediate is asserted.

    blur(image, features, motion, cam, cam_prev, T, ...)          vectorised -> (out [H, W, 3], work dict: plane [H, W, 4], tile, nb [TH, TW, 4])
    blur_scalar(...)                                              the same definition one pixel, one tile, one tap at a time
    handmade_blur_cases(H, W, T, seed)                            hand-made inputs on top of motion_ref.handmade_steps: half-extents from 0 to beyond 16 px
    census(case, T)                                               which regimes a case reaches, counted on the witness alone
Arrays are indexed [i, j, channel] (row, column) and tiles [a, b, channel]: the library's memory is the transpose, pixel (i, j) at slot
j*H + i and tile (a, b) at slot b*TH + a."""
import numpy as np

import denoise_ref as DR
import motion_ref as MR
import temporal_ref as TR

_is = DR._is
bits, same_bits = DR.bits, DR.same_bits
TILE = 16
DEFAULTS = dict(taps=15, shutter=1.0, depth_extent=0.5, gamma=0)
#: the frames (W, H) of the CPU and GPU tests: below one tile, exactly one tile, a one-column second tile, partial tiles, 5 x 3 tiles
SIZES = [(1, 1), (5, 3), (16, 16), (17, 16), (37, 23), (9, 33), (70, 40)]
SEEDS = {np.float32: 83, np.float64: 84}


def _tiles(H, W):
    return (H + TILE - 1) // TILE, (W + TILE - 1) // TILE


def work_elems(H, W):
    TH, TW = _tiles(H, W)
    return (H * W + 2 * TH * TW) * 4


def unpack_work(flat, H, W):
    """the workspace's public layout -> dict plane [H, W, 4], tile, nb [TH, TW, 4]"""
    TH, TW = _tiles(H, W)
    flat = np.asarray(flat).ravel()
    n, t = H * W * 4, TH * TW * 4
    return dict(plane=flat[:n].reshape(W, H, 4).transpose(1, 0, 2), tile=flat[n:n + t].reshape(TW, TH, 4).transpose(1, 0, 2), nb=flat[n + t:n + 2 * t].reshape(TW, TH, 4).transpose(1, 0, 2))


def _clamp01(x, T):
    return np.where(x > T(0), np.where(x < T(1), x, T(1)), T(0))


# ---- vectorised ----------------------------------------------------------------------------------------------------------------------------------
def blur_plane(image, features, motion, cam, cam_prev, T, shutter=1.0, details=None):
    """prepare, previous position, half-extent -> the blur plane [H, W, 4] = (h.x, h.y, zc, l)"""
    T = np.dtype(T).type
    valid, has, _, _, z, _, _ = DR.prepare(image, features, T, False)
    H, W = valid.shape
    K = TR.host_constants(cam_prev, T, 0.1, 0.25, 16.0)
    mv = np.asarray(motion)
    assert mv.shape == (H, W, 4)
    _is(T, mv)
    zero = T(0)
    with np.errstate(all="ignore"):
        rays = MR.centre_rays(cam, W, H, T)
        o, nD = [rays[0, 0, k] for k in range(3)], [rays[..., 3 + k] for k in range(3)]
        po, pw, ph, pv = MR._fields(cam_prev, T, ("origin", "w", "horizontal", "vertical"))
        d = [np.where(has, ((o[k] + z * nD[k]) - mv[..., k]) - po[k], nD[k]) for k in range(3)]
        dot3 = lambda v: (d[0] * v[0] + d[1] * v[1]) + d[2] * v[2]
        dw = dot3(pw)
        front = dw < zero
        lam = K["Kw"] / dw
        s = (lam * dot3(ph) - K["Qh"]) * K["ih"]
        t = (lam * dot3(pv) - K["Qv"]) * K["iv"]
        x = s * T(W) - T(1.5)
        y = (T(H) - T(0.5)) - t * T(H)
        moved = valid & front & np.isfinite(x) & np.isfinite(y)
        jj, ii = np.arange(W, dtype=np.int64).astype(T)[None, :], np.arange(H, dtype=np.int64).astype(T)[:, None]
        ux, uy = np.where(moved, jj - x, zero), np.where(moved, ii - y, zero)
        hs = T(np.float64(shutter) / np.float64(2))
        hx, hy = ux * hs, uy * hs
        l2 = hx * hx + hy * hy
        big = l2 > T(256)
        sc = T(16) / np.sqrt(l2)
        hx, hy = np.where(big, hx * sc, hx), np.where(big, hy * sc, hy)
        l2 = np.where(big, hx * hx + hy * hy, l2)
        l = np.sqrt(l2)
        _is(T, *d, dw, lam, s, t, x, y, ux, uy, hx, hy, l2, sc, l)
    plane = np.empty((H, W, 4), T)
    plane[..., 0], plane[..., 1], plane[..., 3] = hx, hy, l
    plane[..., 2] = np.where(valid, np.where(has, z, T(np.inf)), T(np.nan))
    if details is not None:
        details.update(valid=valid, has=has, front=front, moved=moved, big=big, finite_m=np.isfinite(mv[..., 0:3]).all(axis=-1))
    return plane


def tile_max(plane, details=None):
    """-> [TH, TW, 4] = (h.x, h.y, l, 0) of the pixel with the greatest l of each tile, ties to the lowest slot j*H + i"""
    H, W = plane.shape[:2]
    TH, TW = _tiles(H, W)
    out = np.zeros((TH, TW, 4), plane.dtype)
    ties = 0
    for a in range(TH):
        for b in range(TW):
            sub = plane[a * TILE:(a + 1) * TILE, b * TILE:(b + 1) * TILE]
            lt = sub[..., 3].T                                  # [column, row]: raveled, the order of the slots
            k = int(np.argmax(lt))                              # (the first of equal maxima)
            cj, ci = divmod(k, lt.shape[1])
            out[a, b, 0:2], out[a, b, 2] = sub[ci, cj, 0:2], sub[ci, cj, 3]
            ties += int((lt == lt.ravel()[k]).sum() > 1 and lt.ravel()[k] > 0)
    if details is not None:
        details.update(tile_ties=ties)
    return out


def neighbour_max(tile, details=None):
    """-> [TH, TW, 4] = (vN.x, vN.y, lN, 0): the greatest l over the up to nine tiles around, ties to the lowest tile index b*TH + a"""
    TH, TW = tile.shape[:2]
    T = tile.dtype.type
    best = np.zeros_like(tile)
    best[..., 2] = T(-1)
    src = np.full((TH, TW), -1, np.int64)
    aa, bb = np.meshgrid(np.arange(TH), np.arange(TW), indexing="ij")
    for db in (-1, 0, 1):
        for da in (-1, 0, 1):
            qa, qb = aa + da, bb + db
            inside = (qa >= 0) & (qa < TH) & (qb >= 0) & (qb < TW)
            v = tile[np.clip(qa, 0, TH - 1), np.clip(qb, 0, TW - 1)]
            up = inside & (v[..., 2] > best[..., 2])
            best = np.where(up[..., None], v, best)
            src = np.where(up, qb * TH + qa, src)
    best[..., 3] = 0
    if details is not None:
        details.update(nb_src=src)
    return best


def gather(image, plane, nb, T, taps=15, depth_extent=0.5, gamma=0, details=None):
    T = np.dtype(T).type
    c = np.asarray(image)
    _is(T, c, plane, nb)
    H, W = c.shape[:2]
    one, zero, half = T(1), T(0), T(0.5)
    ext = T(np.float64(depth_extent))
    valid = ~np.isnan(plane[..., 2])
    ii, jj = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    vn = nb[ii // TILE, jj // TILE]
    cnt = dict(taps_outside=0, taps_invalid=0, sphere_over_sky=0, sky_over_sphere=0, both_sky=0, rint_ties=0, soft_depth=0)
    with np.errstate(all="ignore"):
        filt = vn[..., 2] >= half
        zx, lx = plane[..., 2], plane[..., 3]
        lX = np.where(lx > half, lx, half)
        w0 = one / lX
        wsum, acc = w0, c * w0[..., None]
        fj, fi = jj.astype(T), ii.astype(T)
        finx = zx < T(np.inf)
        cone = lambda dist, l: _clamp01(one - dist / l, T)

        def cyl(dist, l):
            xx = _clamp01((dist - T(0.95) * l) / (T(0.1) * l), T)
            r = one - (xx * xx) * (T(3) - T(2) * xx)
            _is(T, xx, r)
            return r
        for n in range(taps):
            if n == (taps - 1) // 2:
                continue
            tt = T(2 * (n + 1) - (taps + 1)) / T(taps + 1)
            pj, pi = fj + vn[..., 0] * tt, fi + vn[..., 1] * tt
            qj, qi = np.rint(pj).astype(np.int64), np.rint(pi).astype(np.int64)
            inside = (qi >= 0) & (qi < H) & (qj >= 0) & (qj < W)
            gi, gj = np.clip(qi, 0, H - 1), np.clip(qj, 0, W - 1)
            sq, cq = plane[gi, gj], c[gi, gj]
            ok = inside & ~np.isnan(sq[..., 2])
            dx, dy = (qj - jj).astype(T), (qi - ii).astype(T)
            dist = np.sqrt(dx * dx + dy * dy)
            lY = np.where(sq[..., 3] > half, sq[..., 3], half)
            zy = sq[..., 2]
            finy, same = zy < T(np.inf), zy == zx
            both = finx & finy
            fa, ba = _clamp01(one - (zy - zx) / ext, T), _clamp01(one - (zx - zy) / ext, T)
            f = np.where(same, one, np.where(both, fa, np.where(finy, one, zero)))
            b = np.where(same, one, np.where(both, ba, np.where(finx, one, zero)))
            a = (f * cone(dist, lY) + b * cone(dist, lX)) + (cyl(dist, lY) * cyl(dist, lX)) * T(2)
            term = a[..., None] * cq
            _is(T, tt, pj, pi, dist, lY, fa, ba, f, b, a, term)
            wsum = np.where(ok, wsum + a, wsum)
            acc = np.where(ok[..., None], acc + term, acc)
            _is(T, wsum, acc)
            live = filt & valid
            cnt["taps_outside"] += int((live & ~inside).sum())
            cnt["taps_invalid"] += int((live & inside & ~ok).sum())
            cnt["sphere_over_sky"] += int((live & ok & finy & ~finx).sum())
            cnt["sky_over_sphere"] += int((live & ok & ~finy & finx).sum())
            cnt["both_sky"] += int((live & ok & ~finy & ~finx).sum())
            cnt["soft_depth"] += int((live & ok & both & ~same).sum())
            cnt["rint_ties"] += int((live & ((np.abs(pj - np.trunc(pj)) == half) | (np.abs(pi - np.trunc(pi)) == half))).sum())
        out = np.where(filt[..., None], acc / wsum[..., None], c)
        if gamma:
            out = np.sqrt(out)
    _is(T, out)
    out[~valid] = np.nan
    if details is not None:
        details.update(cnt, filt=filt)
    return out


def blur(image, features, motion, cam, cam_prev, T, taps=15, shutter=1.0, depth_extent=0.5, gamma=0, details=None):
    """the definition, vectorised -> (out [H, W, 3], dict plane, tile, nb)"""
    plane = blur_plane(image, features, motion, cam, cam_prev, T, shutter, details)
    tile = tile_max(plane, details)
    nb = neighbour_max(tile, details)
    return gather(image, plane, nb, T, taps, depth_extent, gamma, details), dict(plane=plane, tile=tile, nb=nb)


# ---- scalar --------------------------------------------------------------------------------------------------------------------------------------
def _previous_position(i, j, W, H, T, cam_f, prev_f, K, has, z, m):
    """one pixel's (front, x, y): its own ray, the point one frame ago, the projection -- numpy scalars of type T"""
    o, llc, hor, ver = cam_f
    po, pw, ph, pv = prev_f
    dot3 = lambda u, v: (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]
    su = (np.int64(j).astype(T) + T(1.5)) / T(W)
    tv = (np.int64(H - i).astype(T) - T(0.5)) / T(H)
    D = [((llc[k] + su * hor[k]) + tv * ver[k]) - o[k] for k in range(3)]
    sl = np.sqrt(dot3(D, D))
    nD = [D[k] / sl for k in range(3)]
    d = [((o[k] + z * nD[k]) - m[k]) - po[k] for k in range(3)] if has else nD
    dw = dot3(d, pw)
    lam = K["Kw"] / dw
    s = (lam * dot3(d, ph) - K["Qh"]) * K["ih"]
    t = (lam * dot3(d, pv) - K["Qv"]) * K["iv"]
    x = s * T(W) - T(1.5)
    y = (T(H) - T(0.5)) - t * T(H)
    assert all(type(v) is T for v in (su, tv, sl, dw, lam, s, t, x, y, *d))
    return bool(dw < T(0)), x, y


def blur_scalar(image, features, motion, cam, cam_prev, T, taps=15, shutter=1.0, depth_extent=0.5, gamma=0):
    """the same definition, one pixel, one tile and one tap at a time on numpy scalars of type T"""
    T = np.dtype(T).type
    c, f, mv = np.asarray(image), np.asarray(features), np.asarray(motion)
    _is(T, c, f, mv)
    H, W = c.shape[:2]
    TH, TW = _tiles(H, W)
    K = TR.host_constants(cam_prev, T, 0.1, 0.25, 16.0)
    cam_f = MR._fields(cam, T, ("origin", "lower_left_corner", "horizontal", "vertical"))
    prev_f = MR._fields(cam_prev, T, ("origin", "w", "horizontal", "vertical"))
    one, zero, half, inf = T(1), T(0), T(0.5), T(np.inf)
    hs, ext = T(np.float64(shutter) / np.float64(2)), T(np.float64(depth_extent))
    plane = np.zeros((H, W, 4), T)
    tile, nb = np.zeros((TH, TW, 4), T), np.zeros((TH, TW, 4), T)
    out = np.full((H, W, 3), np.nan, T)
    clamp01 = lambda v: (v if v < one else one) if v > zero else zero
    with np.errstate(all="ignore"):
        for i in range(H):
            for j in range(W):
                valid = bool(np.isfinite(c[i, j]).all() and np.isfinite(f[i, j]).all())
                cov = f[i, j, 7]
                has = valid and bool(cov > zero)
                z = f[i, j, 6] / cov if has else zero
                front, x, y = _previous_position(i, j, W, H, T, cam_f, prev_f, K, has, z, mv[i, j])
                moved = valid and front and bool(np.isfinite(x)) and bool(np.isfinite(y))
                hx, hy = ((np.int64(j).astype(T) - x) * hs, (np.int64(i).astype(T) - y) * hs) if moved else (zero * hs, zero * hs)
                l2 = hx * hx + hy * hy
                if l2 > T(256):
                    sc = T(16) / np.sqrt(l2)
                    hx, hy = hx * sc, hy * sc
                    l2 = hx * hx + hy * hy
                l = np.sqrt(l2)
                assert all(type(v) is T for v in (hx, hy, l2, l))
                plane[i, j] = (hx, hy, (z if has else inf) if valid else T(np.nan), l)
        for a in range(TH):
            for b in range(TW):
                best = None
                for j in range(b * TILE, min(W, (b + 1) * TILE)):            # (in the order of the slots: a strictly greater l replaces)
                    for i in range(a * TILE, min(H, (a + 1) * TILE)):
                        if best is None or plane[i, j, 3] > plane[best][3]:
                            best = (i, j)
                tile[a, b] = (plane[best][0], plane[best][1], plane[best][3], zero)
        for a in range(TH):
            for b in range(TW):
                best = None
                for qb in range(max(0, b - 1), min(TW, b + 2)):               # (in the order of the tile index)
                    for qa in range(max(0, a - 1), min(TH, a + 2)):
                        if best is None or tile[qa, qb, 2] > tile[best][2]:
                            best = (qa, qb)
                nb[a, b] = (tile[best][0], tile[best][1], tile[best][2], zero)

        def cone(dist, l):
            return clamp01(one - dist / l)

        def cyl(dist, l):
            xx = clamp01((dist - T(0.95) * l) / (T(0.1) * l))
            return one - (xx * xx) * (T(3) - T(2) * xx)
        for i in range(H):
            for j in range(W):
                zx = plane[i, j, 2]
                if bool(np.isnan(zx)):
                    continue
                vx, vy, lN, _ = nb[i // TILE, j // TILE]
                res = [c[i, j, k] for k in range(3)]
                if lN >= half:
                    lX = plane[i, j, 3] if plane[i, j, 3] > half else half
                    w0 = one / lX
                    wsum, acc = w0, [c[i, j, k] * w0 for k in range(3)]
                    for n in range(taps):
                        if 2 * n == taps - 1:
                            continue
                        tt = T(2 * (n + 1) - (taps + 1)) / T(taps + 1)
                        qj, qi = int(np.rint(np.int64(j).astype(T) + vx * tt)), int(np.rint(np.int64(i).astype(T) + vy * tt))
                        if not (0 <= qi < H and 0 <= qj < W) or bool(np.isnan(plane[qi, qj, 2])):
                            continue
                        dx, dy = np.int64(qj - j).astype(T), np.int64(qi - i).astype(T)
                        dist = np.sqrt(dx * dx + dy * dy)
                        lY = plane[qi, qj, 3] if plane[qi, qj, 3] > half else half
                        zy = plane[qi, qj, 2]
                        if zy == zx:
                            fw, bw = one, one
                        elif zy < inf and zx < inf:
                            fw, bw = clamp01(one - (zy - zx) / ext), clamp01(one - (zx - zy) / ext)
                        elif zy < inf:
                            fw, bw = one, zero
                        else:
                            fw, bw = zero, one
                        a_ = (fw * cone(dist, lY) + bw * cone(dist, lX)) + (cyl(dist, lY) * cyl(dist, lX)) * T(2)
                        assert type(a_) is T and type(tt) is T and type(dist) is T
                        wsum = wsum + a_
                        acc = [acc[k] + a_ * c[qi, qj, k] for k in range(3)]
                    res = [acc[k] / wsum for k in range(3)]
                for k in range(3):
                    assert type(res[k]) is T
                    out[i, j, k] = np.sqrt(res[k]) if gamma else res[k]
    return out, dict(plane=plane, tile=tile, nb=nb)


def same_blur(got, ref):
    return same_bits(got[0], ref[0]) and all(same_bits(got[1][k], ref[1][k]) for k in ("plane", "tile", "nb"))


# ---- hand-made cases and their census --------------------------------------------------------------------------------------------------------
def _plant_exact(case, T, target_u=8.0):
    """Make ONE covered pixel's own displacement u.x exactly `target_u` pixels (so that, with shutter 1, the tile's dominant half-extent is
    exactly target_u / 2 in x and the taps' positions hit exact halves: rint ties).  The pixel's motion slot is m = z * dx * hor / W for a
    real dx found by bisection on the scalar projection, then by single steps of m.x; the first pixel in slot order that admits it is used.
    -> True if one was planted."""
    T = np.dtype(T).type
    image, feat, cam, prev, motion = case["image"], case["features"], case["cam"], case["cam_prev"], case["motion"]
    H, W = image.shape[:2]
    valid, has, _, _, z, _, _ = DR.prepare(image, feat, T, False)
    K = TR.host_constants(prev, T, 0.1, 0.25, 16.0)
    cam_f = MR._fields(cam, T, ("origin", "lower_left_corner", "horizontal", "vertical"))
    prev_f = MR._fields(prev, T, ("origin", "w", "horizontal", "vertical"))
    hor = np.asarray(MR._get(cam, "horizontal")).astype(np.float64)
    tries = 0
    with np.errstate(all="ignore"):
        for j in range(W // 2, W):
            for i in range(H):
                if not has[i, j] or tries >= 12:
                    continue
                tries += 1
                want = np.int64(j).astype(T) - T(target_u)
                m_of = lambda dx: (np.float64(z[i, j]) * dx * hor / W).astype(T)
                x_of = lambda m: _previous_position(i, j, W, H, T, cam_f, prev_f, K, True, z[i, j], m)[1]
                lo, hi = target_u - 1.0, target_u + 1.0
                if not (x_of(m_of(lo)) > want > x_of(m_of(hi))):
                    continue
                for _ in range(80):
                    mid = 0.5 * (lo + hi)
                    xm = x_of(m_of(mid))
                    if xm == want:
                        break
                    lo, hi = (mid, hi) if xm > want else (lo, mid)
                m = m_of(mid)
                if x_of(m) != want:
                    for step in range(1, 40):                    # (the neighbours of m.x, both ways)
                        for sgn in (-np.inf, np.inf):
                            m2 = m.copy()
                            for _ in range(step):
                                m2[0] = np.nextafter(m2[0], T(sgn))
                            if x_of(m2) == want:
                                m = m2
                                break
                        if x_of(m) == want:
                            break
                if x_of(m) == want:
                    motion[i, j, 0:3] = m
                    return True
    return False


def handmade_blur_cases(H, W, T, seed):
    """Hand-made inputs of one frame size on top of motion_ref.handmade_steps (its frames, cameras and motion planes), the planes scaled so that
    the half-extents span 0 to beyond 16 px -> a list of dicts image, features, motion, cam, cam_prev, params:
      0  cam_prev IS cam and the plane is zero but for the columns of the left third (the hand-made plane, halved) and one planted pixel that
         moves by exactly 8 px: pass-through tiles, tiles whose vN comes from a neighbour, rint ties; 15 taps, shutter 1
      1  the second step's moving cameras, the plane times 8: clamped velocities and ties among them; 31 taps, gamma 1
      2  the third step's cameras, the plane as it is, NaN slots included; 5 taps, shutter 0.5, a narrow depth extent"""
    T = np.dtype(T).type
    steps = MR.handmade_steps(H, W, T, seed)
    cases = []
    for k, s in enumerate(steps[:3]):
        motion = s["motion"].copy()
        cam_prev = s["cam_prev"]
        if k == 0:
            cam_prev = s["cam"]
            motion[..., 0:3] = np.where(np.isfinite(motion[..., 0:3]), motion[..., 0:3] * T(0.5), motion[..., 0:3])
            motion[:, (W + 2) // 3:, 0:3] = 0
            params = dict(taps=15, shutter=1.0, depth_extent=0.5, gamma=0)
        elif k == 1:
            motion[..., 0:3] = motion[..., 0:3] * T(8)
            params = dict(taps=31, shutter=1.0, depth_extent=0.5, gamma=1)
        else:
            params = dict(taps=5, shutter=0.5, depth_extent=0.05, gamma=0)
            # one covered pixel whose surface was BEHIND the previous camera one frame ago: m = Pw - origin_prev - w_prev, so d = w_prev and dw > 0
            _, has, _, _, z, _, _ = DR.prepare(s["image"], s["features"], T, False)
            rays = MR.centre_rays(s["cam"], W, H, T).astype(np.float64)
            po, pw = (np.asarray(MR._get(cam_prev, k)).astype(np.float64) for k in ("origin", "w"))
            for i, j in np.argwhere(has & np.isfinite(motion[..., 0:3]).all(axis=-1))[-1:]:
                motion[i, j, 0:3] = ((rays[i, j, 0:3] + np.float64(z[i, j]) * rays[i, j, 3:6]) - po - pw).astype(T)
        case = dict(image=s["image"], features=s["features"], motion=motion, cam=s["cam"], cam_prev=cam_prev, params=params)
        if k == 0:
            case["planted"] = _plant_exact(case, T)
        cases.append(case)
    return cases


def census(case, T):
    """which regimes one case reaches, counted on the witness alone"""
    d = {}
    blur(case["image"], case["features"], case["motion"], case["cam"], case["cam_prev"], T, details=d, **case["params"])
    H, W = d["valid"].shape
    TH, TW = _tiles(H, W)
    own = (np.arange(TW)[None, :] * TH + np.arange(TH)[:, None])
    nbl = neighbour = None
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    filt_tile = np.zeros((TH, TW), bool)
    filt_tile[ii // TILE, jj // TILE] = d["filt"]
    return dict(pass_tiles=int((~filt_tile).sum()), filter_tiles=int(filt_tile.sum()), clamped=int((d["big"] & d["moved"]).sum()),
                from_neighbour=int((d["valid"] & d["filt"] & (d["nb_src"] != own)[ii // TILE, jj // TILE]).sum()), tile_ties=d["tile_ties"],
                taps_outside=d["taps_outside"], taps_invalid=d["taps_invalid"], sphere_over_sky=d["sphere_over_sky"], sky_over_sphere=d["sky_over_sphere"],
                both_sky=d["both_sky"], soft_depth=d["soft_depth"], rint_ties=d["rint_ties"],
                not_front=int((d["valid"] & ~d["front"] & d["finite_m"]).sum()), nan_slot=int((d["valid"] & d["has"] & ~d["finite_m"] & ~d["moved"]).sum()),
                invalid=int((~d["valid"]).sum()))
