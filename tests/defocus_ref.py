"""The witness of the defocus stage (include/rtw_hip.h rtw_defocus_*): the definition restated in numpy, twice -- vectorised over the frame and
one pixel at a time on numpy scalars.  Nothing of the product is used; the frame is prepared by the denoiser's witness and the pixel's own
ray is motion_ref's.  numpy rounds every operation once and never fuses; the element type of every intermediate is asserted.

    defocus(image, features, cam, T, ...)            vectorised -> (out [H, W, 3], work dict: coc [H, W, 4], tile [TH, TW])
    defocus_scalar(...)                              the same definition one pixel, one tile, one tap at a time
    handmade_cases(H, W, T, seed)                    hand-made inputs: values planted on either side of every decision of the definition
    census(case, T)                                  which regimes a case reaches, counted on the witness alone
Arrays are indexed [i, j, channel] (row, column) and tiles [a, b]: the library's memory is the transpose, pixel (i, j) at slot j*H + i and
tile (a, b) at slot b*TH + a."""
import numpy as np

import denoise_ref as DR
import motion_ref as MR

_is = DR._is
bits, same_bits = DR.bits, DR.same_bits
TILE, MAX_RADIUS = 16, 8
DEFAULTS = dict(lens_radius=0.0, focus_dist=0.0, max_radius=8, gamma=0)
#: the frames (W, H) of the GPU test: one pixel, exactly one tile, 2 x 3 and 3 x 2 tiles with a one-pixel last tile, a strip each way, 6 x 4 tiles
SIZES = [(1, 1), (16, 16), (17, 33), (33, 17), (5, 130), (130, 5), (96, 54)]
SEEDS = {np.float32: 91, np.float64: 92}
NEAR = 2.0 ** -10            # "just" below / above a threshold: within this distance of it


class Cam:
    """a camera by its fields (what the library's camera struct holds), arrays of type T"""

    def __init__(self, T, **fields):
        self.elem_type = np.dtype(T).type
        for k, v in fields.items():
            setattr(self, k, np.asarray(v, np.float64).astype(T) if k != "lens_radius" else float(v))


def _tiles(H, W):
    return (H + TILE - 1) // TILE, (W + TILE - 1) // TILE


def work_elems(H, W):
    TH, TW = _tiles(H, W)
    return H * W * 4 + (TH * TW + 3) // 4 * 4


def unpack_work(flat, H, W):
    """the workspace's public layout -> dict coc [H, W, 4], tile [TH, TW]"""
    TH, TW = _tiles(H, W)
    flat = np.asarray(flat).ravel()
    n = H * W * 4
    return dict(coc=flat[:n].reshape(W, H, 4).transpose(1, 0, 2), tile=flat[n:n + TH * TW].reshape(TW, TH).T)


def host_constants(cam, T, W, lens_radius, focus_dist, max_radius):
    """binary64 over the camera's fields, every operation rounded once, then rounded once to T -> F, K, Rm"""
    T = np.dtype(T).type
    o, llc, hor, w = (np.asarray(MR._get(cam, k)).astype(np.float64) for k in ("origin", "lower_left_corner", "horizontal", "w"))
    q = o - llc
    focus = np.float64(focus_dist) if focus_dist > 0 else (q[0] * w[0] + q[1] * w[1]) + q[2] * w[2]
    hh = (hor[0] * hor[0] + hor[1] * hor[1]) + hor[2] * hor[2]
    with np.errstate(all="ignore"):
        K = (np.float64(lens_radius) * np.float64(W)) / np.sqrt(hh)
    return T(focus), T(K), T(max_radius)


def _min(a, b):
    return np.where(a < b, a, b)


def _max(a, b):
    return np.where(a > b, a, b)


def _clamp01(x, T):
    return np.where(x > T(0), np.where(x < T(1), x, T(1)), T(0))


# ---- vectorised ----------------------------------------------------------------------------------------------------------------------------------
def coc_plane(image, features, cam, T, lens_radius=0.0, focus_dist=0.0, max_radius=8, details=None):
    """prepare -> the CoC plane [H, W, 4] = (R, zc, w, 0); (-1, NaN, 0, 0) where the pixel is not valid"""
    T = np.dtype(T).type
    valid, has, _, _, z, _, _ = DR.prepare(image, features, T, False)
    H, W = valid.shape
    F, K, Rm = host_constants(cam, T, W, lens_radius, focus_dist, max_radius)
    (wv,) = MR._fields(cam, T, ("w",))
    half = T(0.5)
    with np.errstate(all="ignore"):
        rays = MR.centre_rays(cam, W, H, T)
        nD = [rays[..., 3 + k] for k in range(3)]
        ca = -((nD[0] * wv[0] + nD[1] * wv[1]) + nD[2] * wv[2])
        zax = z * ca
        Rl = _min(K * (np.abs(zax - F) / zax), Rm)
        Rs = _min(K, Rm)
        lens = has & (zax > T(0))
        R = np.where(lens, Rl, Rs)
        Rh = _max(R, half)
        w = T(1) / (Rh * Rh)
        _is(T, ca, zax, Rl, R, Rh, w)
    plane = np.zeros((H, W, 4), T)
    plane[..., 0] = np.where(valid, R, T(-1))
    plane[..., 1] = np.where(valid, np.where(has, z, T(np.inf)), T(np.nan))
    plane[..., 2] = np.where(valid, w, T(0))
    if details is not None:
        with np.errstate(all="ignore"):
            details.update(valid=valid, has=has, lens=lens, zax=zax, Rm=Rm, K=K, clamped=valid & lens & ~(K * (np.abs(zax - F) / zax) < Rm))
    return plane


def tile_max(plane):
    """-> [TH, TW]: the greatest R of each tile's pixels (-1: none is valid)"""
    H, W = plane.shape[:2]
    TH, TW = _tiles(H, W)
    out = np.empty((TH, TW), plane.dtype)
    for a in range(TH):
        for b in range(TW):
            out[a, b] = plane[a * TILE:(a + 1) * TILE, b * TILE:(b + 1) * TILE, 0].max()
    return out


def neighbour_max(tile):
    """-> [TH, TW]: RN, the maximum over the up to nine tiles around each tile"""
    TH, TW = tile.shape
    out = np.empty_like(tile)
    for a in range(TH):
        for b in range(TW):
            out[a, b] = tile[max(0, a - 1):a + 2, max(0, b - 1):b + 2].max()
    return out


def gather(image, plane, tile, T, gamma=0, details=None):
    T = np.dtype(T).type
    c = np.asarray(image)
    _is(T, c, plane, tile)
    H, W = c.shape[:2]
    half, zero, one = T(0.5), T(0), T(1)
    valid = ~np.isnan(plane[..., 1])
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    RN = neighbour_max(tile)[ii // TILE, jj // TILE]
    names = ("cover0_at", "cover0_above", "cover0_below", "cover1_at", "cover1_below", "cover1_above", "z_equal", "inf_tap", "inf_self", "inf_both", "lim_true", "lim_equal",
             "back_wider_self", "nan_taps", "border_taps")
    cnt = dict.fromkeys(names, 0)
    with np.errstate(all="ignore"):
        filt = RN >= half
        mm = np.where(filt, np.ceil(RN + half) - one, zero).astype(np.int64)
        RX, zX, wX = plane[..., 0], plane[..., 1], plane[..., 2]
        RhX = _max(RX, half)
        wsum, acc = np.zeros((H, W), T), np.zeros((H, W, 3), T)
        mtop = int(mm.max()) if mm.size else 0
        assert mtop <= MAX_RADIUS
        for dj in range(-mtop, mtop + 1):
            for di in range(-mtop, mtop + 1):
                take = filt & (mm >= max(abs(di), abs(dj)))
                if not take.any():
                    continue
                inside = (ii + di >= 0) & (ii + di < H) & (jj + dj >= 0) & (jj + dj < W)
                sq = DR._shift(plane, di, dj, np.nan)
                cq = DR._shift(c, di, dj, 0)
                ok = take & inside & ~np.isnan(sq[..., 1])
                dist = np.sqrt(T(di * di + dj * dj))
                back = sq[..., 1] > zX
                Rhq = _max(sq[..., 0], half)
                lim = back & (RhX < Rhq)
                Re, we = np.where(lim, RhX, Rhq), np.where(lim, wX, sq[..., 2])
                raw = (Re + half) - dist
                cover = _clamp01(raw, T)
                ok = ok & (cover > zero)
                a = cover * we
                term = a[..., None] * cq
                _is(T, dist, Rhq, Re, we, raw, cover, a, term)
                wsum = np.where(ok, wsum + a, wsum)
                acc = np.where(ok[..., None], acc + term, acc)
                _is(T, wsum, acc)
                if details is not None:
                    live = take & valid
                    cnt["border_taps"] += int((live & ~inside).sum())
                    cnt["nan_taps"] += int((live & inside & np.isnan(sq[..., 1])).sum())
                    tap = live & inside & ~np.isnan(sq[..., 1])
                    cnt["cover0_at"] += int((tap & (raw == zero)).sum())
                    cnt["cover0_above"] += int((tap & (raw > zero) & (raw <= T(NEAR))).sum())
                    cnt["cover0_below"] += int((tap & (raw < zero) & (raw >= T(-NEAR))).sum())
                    cnt["cover1_at"] += int((tap & (raw == one)).sum())
                    cnt["cover1_below"] += int((tap & (raw < one) & (raw >= T(1 - NEAR))).sum())
                    cnt["cover1_above"] += int((tap & (raw > one) & (raw <= T(1 + NEAR))).sum())
                    if di or dj:
                        fq, fX = np.isfinite(sq[..., 1]), np.isfinite(zX)
                        cnt["z_equal"] += int((tap & fq & (sq[..., 1] == zX)).sum())
                        cnt["inf_tap"] += int((tap & ~fq & fX).sum())
                        cnt["inf_self"] += int((tap & fq & ~fX).sum())
                        cnt["inf_both"] += int((tap & ~fq & ~fX).sum())
                        cnt["lim_true"] += int((tap & lim).sum())
                        cnt["lim_equal"] += int((tap & back & (RhX == Rhq)).sum())
                        cnt["back_wider_self"] += int((tap & back & (RhX > Rhq)).sum())
        out = np.where(filt[..., None], acc / wsum[..., None], c)
        if gamma:
            out = np.sqrt(out)
    _is(T, out)
    out[~valid] = np.nan
    if details is not None:
        details.update(cnt, filt=filt, RN=RN, m=mm)
    return out


def defocus(image, features, cam, T, lens_radius=0.0, focus_dist=0.0, max_radius=8, gamma=0, details=None):
    """the definition, vectorised -> (out [H, W, 3], dict coc, tile)"""
    plane = coc_plane(image, features, cam, T, lens_radius, focus_dist, max_radius, details)
    tile = tile_max(plane)
    return gather(image, plane, tile, T, gamma, details), dict(coc=plane, tile=tile)


# ---- scalar --------------------------------------------------------------------------------------------------------------------------------------
def defocus_scalar(image, features, cam, T, lens_radius=0.0, focus_dist=0.0, max_radius=8, gamma=0):
    """the same definition, one pixel, one tile and one tap at a time on numpy scalars of type T"""
    T = np.dtype(T).type
    c, f = np.asarray(image), np.asarray(features)
    _is(T, c, f)
    H, W = c.shape[:2]
    TH, TW = _tiles(H, W)
    F, K, Rm = host_constants(cam, T, W, lens_radius, focus_dist, max_radius)
    o, llc, hor, ver, wv = MR._fields(cam, T, ("origin", "lower_left_corner", "horizontal", "vertical", "w"))
    one, zero, half, inf = T(1), T(0), T(0.5), T(np.inf)
    dot3 = lambda u, v: (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]
    plane = np.zeros((H, W, 4), T)
    tile = np.full((TH, TW), -1, T)
    out = np.full((H, W, 3), np.nan, T)
    with np.errstate(all="ignore"):
        for i in range(H):
            for j in range(W):
                if not (np.isfinite(c[i, j]).all() and np.isfinite(f[i, j]).all()):
                    plane[i, j] = (T(-1), T(np.nan), zero, zero)
                    continue
                cov = f[i, j, 7]
                has = bool(cov > zero)
                z = f[i, j, 6] / cov if has else zero
                su = (np.int64(j).astype(T) + T(1.5)) / T(W)
                tv = (np.int64(H - i).astype(T) - T(0.5)) / T(H)
                D = [((llc[k] + su * hor[k]) + tv * ver[k]) - o[k] for k in range(3)]
                sl = np.sqrt(dot3(D, D))
                nD = [D[k] / sl for k in range(3)]
                ca = -dot3(nD, wv)
                zax = z * ca
                if has and zax > zero:
                    r = K * (np.abs(zax - F) / zax)
                    R = r if r < Rm else Rm
                else:
                    R = K if K < Rm else Rm
                Rh = R if R > half else half
                w = one / (Rh * Rh)
                assert all(type(v) is T for v in (z, su, tv, sl, ca, zax, R, Rh, w))
                plane[i, j] = (R, z if has else inf, w, zero)
                if R > tile[i // TILE, j // TILE]:
                    tile[i // TILE, j // TILE] = R
        for i in range(H):
            for j in range(W):
                RX, zX, wX, _ = plane[i, j]
                if np.isnan(zX):
                    continue
                a0, b0 = i // TILE, j // TILE
                RN = T(-1)
                for qb in range(max(0, b0 - 1), min(TW, b0 + 2)):
                    for qa in range(max(0, a0 - 1), min(TH, a0 + 2)):
                        RN = tile[qa, qb] if tile[qa, qb] > RN else RN
                res = [c[i, j, k] for k in range(3)]
                if RN >= half:
                    m = int(np.ceil(RN + half)) - 1
                    RhX = RX if RX > half else half
                    wsum, acc = zero, [zero, zero, zero]
                    for dj in range(-m, m + 1):
                        for di in range(-m, m + 1):
                            qi, qj = i + di, j + dj
                            if not (0 <= qi < H and 0 <= qj < W) or np.isnan(plane[qi, qj, 1]):
                                continue
                            Rq, zq, wq, _ = plane[qi, qj]
                            dist = np.sqrt(T(di * di + dj * dj))
                            Rhq = Rq if Rq > half else half
                            lim = bool(zq > zX) and bool(RhX < Rhq)
                            Re, we = (RhX, wX) if lim else (Rhq, wq)
                            cover = (Re + half) - dist
                            cover = (cover if cover < one else one) if cover > zero else zero
                            if not cover > zero:
                                continue
                            a = cover * we
                            assert type(a) is T and type(dist) is T
                            wsum = wsum + a
                            acc = [acc[k] + a * c[qi, qj, k] for k in range(3)]
                    res = [acc[k] / wsum for k in range(3)]
                for k in range(3):
                    assert type(res[k]) is T
                    out[i, j, k] = np.sqrt(res[k]) if gamma else res[k]
    return out, dict(coc=plane, tile=tile)


def same_defocus(got, ref):
    """the image and both planes of the workspace on the bits, NaNs equal as NaNs"""
    return same_bits(got[0], ref[0]) and all(same_bits(got[1][k], ref[1][k]) for k in ("coc", "tile"))


# ---- hand-made cases and their census --------------------------------------------------------------------------------------------------------
def handmade_camera(H, W, T, focus=4.0, origin=(0.5, -0.25, 1.0)):
    """A camera whose horizontal vector is exactly W/8 long, so that K = (lens_radius*W) / (W/8) is exact for a lens_radius of target/8:
    looking down -z from `origin`, the focus plane `focus` away"""
    o, w = np.array(origin, np.float64), np.array([0.0, 0.0, 1.0])
    hor, ver = np.array([W / 8.0, 0.0, 0.0]), np.array([0.0, H / 8.0, 0.0])
    return Cam(T, origin=o, lower_left_corner=o - hor / 2 - ver / 2 - focus * w, horizontal=hor, vertical=ver, u=[1, 0, 0], v=[0, 1, 0], w=w, lens_radius=0.0)


def lens_for(cam, T, W, target):
    """a lens_radius whose K is exactly `target` (a value of type T): target/8 by construction, else the nearest of the doubles around it"""
    T = np.dtype(T).type
    lr = np.float64(target) / np.float64(8)
    best = lr
    for step in range(0, 400):
        for sgn in (1, -1):
            x = lr
            for _ in range(step):
                x = np.nextafter(x, np.float64(sgn) * np.inf)
            k = host_constants(cam, T, W, x, 0.0, 8)[1]
            if k == T(target):
                return float(x)
            if abs(np.float64(k) - np.float64(target)) < abs(np.float64(host_constants(cam, T, W, best, 0.0, 8)[1]) - np.float64(target)):
                best = x
        if step > 8 and T is np.float32:
            break
    return float(best)


def _plant_depth(cam, T, H, W, K, F, target, below):
    """per pixel, on the far side of the focus plane, the least depth z (a value of T; cov = 1: z is feature 6 itself) whose R = K*(|zax - F|/zax)
    is >= target[i, j] -- by bisection on the bit patterns, R is monotone in z there; below[i, j]: the float just under it (R < target)"""
    T = np.dtype(T).type
    I = np.int32 if T is np.float32 else np.int64
    (wv,) = MR._fields(cam, T, ("w",))
    with np.errstate(all="ignore"):
        rays = MR.centre_rays(cam, W, H, T)
        ca = -((rays[..., 3] * wv[0] + rays[..., 4] * wv[1]) + rays[..., 5] * wv[2])
        R_of = lambda z: K * (np.abs(z * ca - F) / (z * ca))
        lo = (np.full((H, W), F, T) / ca * T(1.0001)).astype(T)        # (just behind the focus plane: R about 0)
        hi = np.full((H, W), 1e6, T)
        lo_b, hi_b = lo.view(I).copy(), hi.view(I).copy()
        for _ in range(70):
            mid = lo_b + (hi_b - lo_b) // 2
            ge = R_of(mid.view(T)) >= target
            hi_b = np.where(ge, mid, hi_b)
            lo_b = np.where(ge, lo_b, mid)
        z = np.where(below, lo_b, hi_b).astype(I).view(T)
    return z


def handmade_cases(H, W, T, seed):
    """Hand-made inputs of one frame size -> a list of dicts image, features, cam, params (lens_radius, focus_dist, max_radius, gamma).  The
    camera is handmade_camera; depths are planted by bisection (_plant_depth), apertures by construction (lens_for).  The tiles furthest along
    the frame's longer axis are the FAR tiles, the others the NEAR ones.
      0 - 2  K is the float just under 1/2, exactly 1/2, just over it; sky pixels (R = K) among surfaces behind the focus plane (R < K): RN just
             below / at / above 1/2 -- everything passes through; m = 0; m = 1
      3 - 5  K just under 3/2, exactly 3/2, just over; max_radius 3; sky, surfaces on both sides of the focus plane (near ones up to the clamp),
             blocks of equal depth, depths <= 0, pixels that are not finite: cover at dist = Re + 1/2 (dist 2) and Re - 1/2 (dist 1) from either side
      6 - 12 max_radius = k for k = 1 .. 7, K = 12: sky and near surfaces sit at the clamp Rm = k, so m = k; planted radii d - 1/2 and d + 1/2
             for the lattice distances d, found by bisection; odd k: a focus override and gamma 1
      13     max_radius 8, K = 12: the FAR tiles as in 6 - 12, the NEAR tiles hold only surfaces with R planted just under 1/2 -- tiles next to a
             far tile filter because of a radius that exists only in the neighbouring tile, the others pass"""
    T = np.dtype(T).type
    rng = np.random.default_rng(seed + 1000 * H + W)
    cam = handmade_camera(H, W, T)
    TH, TW = _tiles(H, W)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    far = (jj // TILE == TW - 1) if W >= H else (ii // TILE == TH - 1)
    cases = []
    half = T(0.5)

    def frame(z, cov):
        albedo = rng.uniform(0.05, 1.0, size=(H, W, 3))
        v = rng.normal(size=(H, W, 3))
        v /= np.linalg.norm(v, axis=2, keepdims=True)
        image = (albedo * rng.uniform(0.0, 2.0, size=(H, W, 1)) * rng.uniform(0.5, 1.5, size=(H, W, 3))).astype(T)
        feat = np.concatenate([albedo, v * cov[..., None], np.zeros((H, W, 1)), cov[..., None]], axis=2).astype(T)
        feat[..., 6] = np.where(cov > 0, z, T(0))                # (cov is 0 or 1 here: depth*cov is the planted depth itself)
        return image, feat

    def poison(image, feat):
        if H * W >= 12:
            for n, (arr, ch, val) in enumerate(((image, 1, np.nan), (feat, 7, np.inf), (feat, 4, -np.inf), (image, 0, np.inf))):
                i, j = (0, int(rng.integers(W))) if n == 0 else (int(rng.integers(H)), int(rng.integers(W)))
                arr[i, j, ch] = val

    def planted(K, F, lo_t, hi_t, palette, p_palette):
        """targets: uniform in [lo_t, hi_t), a share p_palette of the pixels from `palette` (value, below) pairs"""
        target = rng.uniform(lo_t, hi_t, size=(H, W)).astype(T)
        below = np.zeros((H, W), bool)
        pick = rng.random((H, W)) < p_palette
        idx = rng.integers(len(palette), size=(H, W))
        for n, (val, bl) in enumerate(palette):
            sel = pick & (idx == n)
            target = np.where(sel, T(val), target)
            below = np.where(sel, bl, below)
        return _plant_depth(cam, T, H, W, K, F, target, below)

    # ---- 0 - 2: RN around 1/2
    for tgt in (np.nextafter(half, T(0)), half, np.nextafter(half, T(1))):
        lr = lens_for(cam, T, W, tgt)
        F, K, _ = host_constants(cam, T, W, lr, 0.0, 8)
        z = planted(K, F, 0.0, 0.45, [(0.3, False)], 0.2)
        cov = np.where(far & (rng.random((H, W)) < 0.3), 0.0, 1.0)
        image, feat = frame(z, cov)
        cases.append(dict(image=image, features=feat, cam=cam, params=dict(lens_radius=lr, focus_dist=0.0, max_radius=8, gamma=int(len(cases) == 0))))
    # ---- 3 - 5: cover around 0 and 1 by sky pixels of radius 3/2
    tq = T(1.5)
    for tgt in (np.nextafter(tq, T(0)), tq, np.nextafter(tq, T(2))):
        lr = lens_for(cam, T, W, tgt)
        F, K, _ = host_constants(cam, T, W, lr, 0.0, 3)
        z = planted(K, F, 0.0, 1.4, [(0.5, False), (0.5, True), (1.0, False)], 0.3)
        near = rng.random((H, W)) < 0.2                          # in front of the focus plane: R = K*(F - zax)/zax, up to the clamp
        z = np.where(near, (F * rng.uniform(0.05, 0.9, size=(H, W))).astype(T), z)
        z = np.where(rng.random((H, W)) < 0.04, T(0) - z * (rng.random((H, W)) < 0.5), z).astype(T)        # zax <= 0: negative or exactly 0
        for _ in range(2):                                       # blocks of one depth: zc_q == zc_X
            i0, j0 = int(rng.integers(max(1, H - 3))), int(rng.integers(max(1, W - 3)))
            z[i0:i0 + 4, j0:j0 + 4] = z[i0, j0]
        cov = np.where(rng.random((H, W)) < 0.3, 0.0, 1.0)
        image, feat = frame(z, cov)
        poison(image, feat)
        cases.append(dict(image=image, features=feat, cam=cam, params=dict(lens_radius=lr, focus_dist=0.0, max_radius=3, gamma=0)))
    # ---- 6 - 13: m = 1 .. 8
    dists = sorted({float(np.sqrt(T(a * a + b * b))) for a in range(0, 9) for b in range(0, 9) if a or b})
    for k in range(1, 9):
        fd = 6.0 if k % 2 else 0.0
        lr = lens_for(cam, T, W, T(12))
        F, K, Rm = host_constants(cam, T, W, lr, fd, k)
        palette = [(d - 0.5, bl) for d in dists if 0.5 < d - 0.5 < k for bl in (False, True)] + [(d + 0.5, bl) for d in dists if d + 0.5 < k for bl in (False, True)] + [(0.5, True)]
        z = planted(K, F, 0.0, min(float(k), 9.0), palette, 0.5)
        near = rng.random((H, W)) < 0.15
        z = np.where(near, (F * rng.uniform(0.05, 0.9, size=(H, W))).astype(T), z)
        cov = np.where(rng.random((H, W)) < 0.15, 0.0, 1.0)
        if k == 8:
            calm = planted(K, F, 0.0, 0.45, [(0.5, True)], 0.3)
            z, cov = np.where(far, z, calm), np.where(far, cov, 1.0)
        image, feat = frame(z.astype(T), cov)
        poison(image, feat)
        cases.append(dict(image=image, features=feat, cam=cam, params=dict(lens_radius=lr, focus_dist=fd, max_radius=k, gamma=k % 2)))
    return cases


REGIMES = ["rn_below", "rn_at", "rn_above", "cover0_at", "cover0_above", "cover0_below", "cover1_at", "cover1_below", "cover1_above", "z_equal", "inf_tap", "inf_self", "inf_both",
           "lim_true", "lim_equal", "back_wider_self", "zax_le_0", "clamped", "nan_taps", "border_taps", "neighbour_only", "invalid"] + [f"m{k}" for k in range(9)]


def census(case, T):
    """which regimes one case reaches, counted on the witness alone (pixels or taps)"""
    T = np.dtype(T).type
    d = {}
    _, work = defocus(case["image"], case["features"], case["cam"], T, details=d, **case["params"])
    valid, RN, half = d["valid"], d["RN"], T(0.5)
    H, W = valid.shape
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    own = work["tile"][ii // TILE, jj // TILE]
    out = {k: d[k] for k in REGIMES if k in d and np.ndim(d[k]) == 0}
    with np.errstate(all="ignore"):
        out.update(rn_below=int((valid & (RN < half) & (RN >= half - T(NEAR))).sum()), rn_at=int((valid & (RN == half)).sum()),
                   rn_above=int((valid & (RN > half) & (RN <= half + T(NEAR))).sum()), zax_le_0=int((valid & d["has"] & ~(d["zax"] > 0)).sum()),
                   clamped=int(d["clamped"].sum()), neighbour_only=int((valid & d["filt"] & (own < half)).sum()), invalid=int((~valid).sum()))
    for k in range(9):
        out[f"m{k}"] = int((valid & d["filt"] & (d["m"] == k)).sum())
    return out
