"""The witness of the wide-aperture stage (include/rtw_hip.h rtw_wide_aperture_*): the definition restated in numpy, twice -- vectorised over the
frame (on top of the defocus stage's vectorised witness, tests/defocus_ref.py, for the steps that ARE that stage) and one pixel, one block and
one tap at a time on numpy scalars (nothing shared with the vectorised form but the host constants).  Nothing of the product is used.  numpy
rounds every operation once and never fuses; the element type of every intermediate is asserted.

    wide_aperture(image, features, cam, T, ...)      vectorised -> (out [H, W, 3], work dict of every workspace region)
    wide_aperture_scalar(...)                        the same definition one pixel, one block, one tap at a time
    handmade_cases(H, W, T, seed)                    hand-made inputs: values planted on either side of every decision of the definition
    census(case, T)                                  which regimes a case reaches, counted on the witness alone
Arrays are indexed [i, j, channel] (row, column), tiles [a, b]: the library's memory is the transpose (defocus_ref).  The work dict of a call
with max_radius <= 8 is the defocus stage's (coc, tile); otherwise n_coc, n_tile (the narrow stage's planes), coc, tile (the wide ones),
narrow (N), lo_image, lo_coc, lo_tile, lo_out (O)."""
import numpy as np

import defocus_ref as FO
import motion_ref as MR

_is = FO._is
bits, same_bits = FO.bits, FO.same_bits
TILE, MAX_RADIUS, NARROW = 16, 32, 8
SIZES = FO.SIZES
#: the frames (W, H) of the CPU tests: the GPU test's two with partial blocks and a one-pixel last tile, and one whose last block is whole
CPU_SIZES = [(17, 33), (33, 17), (16, 16)]
SEEDS = {np.float32: 191, np.float64: 192}
NEAR = FO.NEAR
REGIONS = ("n_coc", "n_tile", "coc", "tile", "narrow", "lo_image", "lo_coc", "lo_tile", "lo_out")


def scale_of(max_radius):
    return 1 if max_radius <= 8 else (2 if max_radius <= 16 else 4)


def small_size(H, W, s):
    return (H + s - 1) // s, (W + s - 1) // s


def _r4(n):
    return (n + 3) // 4 * 4


def layout(H, W, max_radius):
    """the workspace's public layout in ELEMENTS -> (dict name -> (offset, count, shape in the library's memory order), total)"""
    s = scale_of(max_radius)
    TH, TW = FO._tiles(H, W)
    if s == 1:
        return dict(coc=(0, H * W * 4, (W, H, 4)), tile=(H * W * 4, TH * TW, (TW, TH))), FO.work_elems(H, W)
    h, w = small_size(H, W, s)
    th, tw = FO._tiles(h, w)
    out, at = {}, 0
    for name, count, pad, shape in (("n_coc", H * W * 4, H * W * 4, (W, H, 4)), ("n_tile", TH * TW, _r4(TH * TW), (TW, TH)), ("coc", H * W * 4, H * W * 4, (W, H, 4)),
                                    ("tile", TH * TW, _r4(TH * TW), (TW, TH)), ("narrow", H * W * 3, _r4(H * W * 3), (W, H, 3)), ("lo_image", h * w * 3, _r4(h * w * 3), (w, h, 3)),
                                    ("lo_coc", h * w * 4, h * w * 4, (w, h, 4)), ("lo_tile", th * tw, _r4(th * tw), (tw, th)), ("lo_out", h * w * 3, _r4(h * w * 3), (w, h, 3))):
        out[name] = (at, count, shape)
        at += pad
    return out, at


def work_elems(H, W, max_radius):
    return layout(H, W, max_radius)[1]


def unpack_work(flat, H, W, max_radius):
    """the workspace as the library leaves it -> the work dict, arrays indexed [row, column(, channel)]"""
    flat = np.asarray(flat).ravel()
    out = {}
    for name, (at, count, shape) in layout(H, W, max_radius)[0].items():
        a = flat[at:at + count].reshape(shape)
        out[name] = a.transpose(1, 0, 2) if a.ndim == 3 else a.T
    return out


# ---- vectorised ----------------------------------------------------------------------------------------------------------------------------------
def reduce_frame(image, plane, s, T, details=None):
    """step 4 -> lo_image [h, w, 3], lo_coc [h, w, 4]"""
    T = np.dtype(T).type
    c = np.asarray(image)
    _is(T, c, plane)
    H, W = c.shape[:2]
    h, w = small_size(H, W, s)
    pc = np.zeros((h * s, w * s, 3), T)
    pp = np.full((h * s, w * s, 4), np.nan, T)
    inside = np.zeros((h * s, w * s), bool)
    pc[:H, :W], pp[:H, :W], inside[:H, :W] = c, plane, True
    csum, rsum, zmin, n = np.zeros((h, w, 3), T), np.zeros((h, w), T), np.full((h, w), np.inf, T), np.zeros((h, w), np.int64)
    n_in, n_clamp, n_sky = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    with np.errstate(all="ignore"):
        for dc in range(s):
            for dr in range(s):
                q, cq = pp[dr::s, dc::s], pc[dr::s, dc::s]
                ok = inside[dr::s, dc::s] & ~np.isnan(q[..., 1])
                csum = np.where(ok[..., None], csum + cq, csum)
                rsum = np.where(ok, rsum + q[..., 0], rsum)
                zmin = np.where(ok & (q[..., 1] < zmin), q[..., 1], zmin)
                n += ok
                n_in += inside[dr::s, dc::s]
                n_sky += ok & np.isinf(q[..., 1])
                if details is not None:
                    n_clamp += ok & (q[..., 0] == details["Rm"])
        any_ = n > 0
        cnt = np.where(any_, n, 1).astype(T)
        Rs = (rsum / cnt) * T(1.0 / s)
        Rh = FO._max(Rs, T(0.5))
        ws = T(1) / (Rh * Rh)
        lo_image = np.where(any_[..., None], csum / cnt[..., None], T(0))
        _is(T, csum, rsum, zmin, cnt, Rs, Rh, ws, lo_image)
    lo_coc = np.zeros((h, w, 4), T)
    lo_coc[..., 0] = np.where(any_, Rs, T(-1))
    lo_coc[..., 1] = np.where(any_, zmin, T(np.nan))
    lo_coc[..., 2] = np.where(any_, ws, T(0))
    if details is not None:
        details.update(block_n=n, block_in=n_in, block_clamp=n_clamp, block_sky=n_sky)
    return lo_image, lo_coc


def compose(plane, narrow, lo_coc, lo_out, s, T, gamma=0, details=None):
    """step 6 -> out [H, W, 3]"""
    T = np.dtype(T).type
    _is(T, plane, narrow, lo_coc, lo_out)
    H, W = plane.shape[:2]
    h, w = lo_coc.shape[:2]
    lo_valid = ~np.isnan(lo_coc[..., 1])
    u, v = 2 * np.arange(H) + 1 - s, 2 * np.arange(W) + 1 - s
    a0, b0 = np.floor_divide(u, 2 * s), np.floor_divide(v, 2 * s)
    fy, fx = (u - 2 * s * a0).astype(T) / T(2 * s), (v - 2 * s * b0).astype(T) / T(2 * s)
    wy, wx = (T(1) - fy, fy), (T(1) - fx, fx)
    ws, acc = np.zeros((H, W), T), np.zeros((H, W, 3), T)
    skipped = np.zeros((H, W), np.int64)
    with np.errstate(all="ignore"):
        for c in range(2):
            for r in range(2):
                ra, cb = np.clip(a0 + r, 0, h - 1), np.clip(b0 + c, 0, w - 1)
                ok = lo_valid[ra[:, None], cb[None, :]]
                wt = wy[r][:, None] * wx[c][None, :]
                term = wt[..., None] * lo_out[ra[:, None], cb[None, :]]
                _is(T, wt, term)
                ws = np.where(ok, ws + wt, ws)
                acc = np.where(ok[..., None], acc + term, acc)
                skipped += ~ok
        U = acc / ws[..., None]
        t = FO._clamp01((plane[..., 0] - T(4)) * T(0.25), T)
        mix = narrow + t[..., None] * (U - narrow)
        out = np.where((t <= T(0))[..., None], narrow, np.where((t >= T(1))[..., None], U, mix))
        _is(T, ws, acc, U, t, mix, out)
        if gamma:
            out = np.sqrt(out)
    _is(T, out)
    valid = ~np.isnan(plane[..., 1])
    out[~valid] = np.nan
    if details is not None:
        details.update(t=t, a0=a0, b0=b0, skipped=np.where(valid, skipped, 0), ws=ws)
    return out


def wide_aperture(image, features, cam, T, lens_radius=0.0, focus_dist=0.0, max_radius=32, gamma=0, details=None):
    """the definition, vectorised -> (out [H, W, 3], the work dict)"""
    T = np.dtype(T).type
    s = scale_of(max_radius)
    if s == 1:
        return FO.defocus(image, features, cam, T, lens_radius, focus_dist, max_radius, gamma, details)
    narrow, nw = FO.defocus(image, features, cam, T, lens_radius, focus_dist, NARROW, 0)
    d = {} if details is None else details
    plane = FO.coc_plane(image, features, cam, T, lens_radius, focus_dist, max_radius, d)
    tile = FO.tile_max(plane)
    lo_image, lo_coc = reduce_frame(image, plane, s, T, d)
    lo_tile = FO.tile_max(lo_coc)
    g = {}
    lo_out = FO.gather(lo_image, lo_coc, lo_tile, T, 0, g)
    assert int(g["m"].max()) <= (max_radius + s - 1) // s
    d.update(lo_m=g["m"], lo_filt=g["filt"])
    out = compose(plane, narrow, lo_coc, lo_out, s, T, gamma, d)
    return out, dict(n_coc=nw["coc"], n_tile=nw["tile"], coc=plane, tile=tile, narrow=narrow, lo_image=lo_image, lo_coc=lo_coc, lo_tile=lo_tile, lo_out=lo_out)


# ---- scalar --------------------------------------------------------------------------------------------------------------------------------------
def _prepare_scalar(c, f, cam, T, F, K, Rm):
    """Prepare and Tile max of the defocus block, one pixel at a time -> plane [H, W, 4], tile [TH, TW]"""
    H, W = c.shape[:2]
    TH, TW = FO._tiles(H, W)
    o, llc, hor, ver, wv = MR._fields(cam, T, ("origin", "lower_left_corner", "horizontal", "vertical", "w"))
    one, zero, half, inf = T(1), T(0), T(0.5), T(np.inf)
    dot3 = lambda p, q: (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]
    plane, tile = np.zeros((H, W, 4), T), np.full((TH, TW), -1, T)
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
            zax = z * (-dot3(nD, wv))
            if has and zax > zero:
                r = K * (np.abs(zax - F) / zax)
                R = r if r < Rm else Rm
            else:
                R = K if K < Rm else Rm
            Rh = R if R > half else half
            w = one / (Rh * Rh)
            assert all(type(x) is T for x in (z, zax, R, Rh, w))
            plane[i, j] = (R, z if has else inf, w, zero)
            if R > tile[i // TILE, j // TILE]:
                tile[i // TILE, j // TILE] = R
    return plane, tile


def _gather_scalar(c, plane, tile, T):
    """Gather of the defocus block with gamma 0 on a frame of any size, one pixel and one tap at a time"""
    H, W = c.shape[:2]
    TH, TW = tile.shape
    one, zero, half = T(1), T(0), T(0.5)
    out = np.full((H, W, 3), np.nan, T)
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
                assert m <= NARROW
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
                out[i, j, k] = res[k]
    return out


def wide_aperture_scalar(image, features, cam, T, lens_radius=0.0, focus_dist=0.0, max_radius=32, gamma=0):
    """the same definition, one pixel, one block and one tap at a time on numpy scalars of type T"""
    T = np.dtype(T).type
    c, f = np.asarray(image), np.asarray(features)
    _is(T, c, f)
    H, W = c.shape[:2]
    s = scale_of(max_radius)
    F, K, Rm = FO.host_constants(cam, T, W, lens_radius, focus_dist, max_radius)
    one, zero, half = T(1), T(0), T(0.5)
    with np.errstate(all="ignore"):
        if s == 1:
            plane, tile = _prepare_scalar(c, f, cam, T, F, K, Rm)
            out = _gather_scalar(c, plane, tile, T)
            return (np.sqrt(out) if gamma else out), dict(coc=plane, tile=tile)
        n_coc, n_tile = _prepare_scalar(c, f, cam, T, F, K, T(NARROW))
        narrow = _gather_scalar(c, n_coc, n_tile, T)
        plane, tile = _prepare_scalar(c, f, cam, T, F, K, Rm)
        # ---- reduce
        h, w = small_size(H, W, s)
        th, tw = FO._tiles(h, w)
        lo_image, lo_coc, lo_tile = np.zeros((h, w, 3), T), np.zeros((h, w, 4), T), np.full((th, tw), -1, T)
        inv_s = T(1.0 / s)
        for a in range(h):
            for b in range(w):
                csum, rsum, zmin, n = [zero, zero, zero], zero, T(np.inf), 0
                for j in range(s * b, min(s * b + s, W)):
                    for i in range(s * a, min(s * a + s, H)):
                        R, zc = plane[i, j, 0], plane[i, j, 1]
                        if np.isnan(zc):
                            continue
                        csum = [csum[k] + c[i, j, k] for k in range(3)]
                        rsum = rsum + R
                        zmin = zc if zc < zmin else zmin
                        n += 1
                if n == 0:
                    lo_coc[a, b] = (T(-1), T(np.nan), zero, zero)
                    continue
                cnt = T(n)
                Rs = (rsum / cnt) * inv_s
                Rh = Rs if Rs > half else half
                ws = one / (Rh * Rh)
                assert all(type(x) is T for x in (Rs, Rh, ws, rsum, zmin, *csum))
                lo_image[a, b] = [csum[k] / cnt for k in range(3)]
                lo_coc[a, b] = (Rs, zmin, ws, zero)
                if Rs > lo_tile[a // TILE, b // TILE]:
                    lo_tile[a // TILE, b // TILE] = Rs
        lo_out = _gather_scalar(lo_image, lo_coc, lo_tile, T)
        # ---- compose
        out = np.full((H, W, 3), np.nan, T)
        four, quarter, two_s = T(4), T(0.25), T(2 * s)
        for i in range(H):
            for j in range(W):
                if np.isnan(plane[i, j, 1]):
                    continue
                u, v = 2 * i + 1 - s, 2 * j + 1 - s
                a0, b0 = u // (2 * s), v // (2 * s)
                fy, fx = T(u - 2 * s * a0) / two_s, T(v - 2 * s * b0) / two_s
                rows = ((min(max(a0, 0), h - 1), one - fy), (min(max(a0 + 1, 0), h - 1), fy))
                cols = ((min(max(b0, 0), w - 1), one - fx), (min(max(b0 + 1, 0), w - 1), fx))
                ws, acc = zero, [zero, zero, zero]
                for cb, wxc in cols:
                    for ra, wyr in rows:
                        if np.isnan(lo_coc[ra, cb, 1]):
                            continue
                        wt = wyr * wxc
                        assert type(wt) is T
                        ws = ws + wt
                        acc = [acc[k] + wt * lo_out[ra, cb, k] for k in range(3)]
                assert ws > zero
                t = (plane[i, j, 0] - four) * quarter
                t = (t if t < one else one) if t > zero else zero
                for k in range(3):
                    N, U = narrow[i, j, k], acc[k] / ws
                    res = N if t <= zero else (U if t >= one else N + t * (U - N))
                    assert type(res) is T
                    out[i, j, k] = np.sqrt(res) if gamma else res
    return out, dict(n_coc=n_coc, n_tile=n_tile, coc=plane, tile=tile, narrow=narrow, lo_image=lo_image, lo_coc=lo_coc, lo_tile=lo_tile, lo_out=lo_out)


def same_result(got, ref):
    """the image and every region of the workspace on the bits, NaNs equal as NaNs"""
    return same_bits(got[0], ref[0]) and set(got[1]) == set(ref[1]) and all(same_bits(got[1][k], ref[1][k]) for k in ref[1])


# ---- hand-made cases and their census --------------------------------------------------------------------------------------------------------
#: (max_radius, K): the six clamps of the issue under an aperture far beyond them (sky and near surfaces sit at Rm), then max_radius 16 under
#: apertures whose sky radius K is exactly 2, 4, 6, 8, 10, 14 px with nothing in front of the focus plane: the small frame's m is K/2 (1 .. 7)
CASE_PARAMS = [(9, 40), (12, 40), (16, 40), (17, 40), (24, 40), (32, 40), (16, 2), (16, 4), (16, 6), (16, 8), (16, 10), (16, 14)]


def handmade_cases(H, W, T, seed):
    """Hand-made inputs of one frame size -> a list of dicts image, features, cam, params (lens_radius, focus_dist, max_radius, gamma), one per
    entry of CASE_PARAMS.  The camera is defocus_ref.handmade_camera; depths behind the focus plane are planted by bisection
    (defocus_ref._plant_depth) on radii uniform in [0, min(K, Rm)) with a palette of the blend's thresholds: 4 and 8, each reached from
    either side.  Sky comes in whole 4 x 4-aligned squares (blocks whose least depth is +inf and, with K = 40, blocks that sit at the clamp
    pixel for pixel) and in single pixels; with K = 40 a share of the surfaces lies in front of the focus plane, up to the clamp.  Pixels
    that are not finite come singly (blocks that are partly valid) and in whole 4 x 4-aligned squares (blocks with no valid pixel).  Odd
    cases carry a focus override and gamma 1."""
    T = np.dtype(T).type
    rng = np.random.default_rng(seed + 1000 * H + W)
    cam = FO.handmade_camera(H, W, T)
    cases = []
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")

    def squares(share):
        """a mask of whole 4 x 4-aligned squares, each taken with probability `share`"""
        pick = rng.random(((H + 3) // 4, (W + 3) // 4)) < share
        return pick[ii // 4, jj // 4]

    for n, (max_radius, k_px) in enumerate(CASE_PARAMS):
        fd = 6.0 if n % 2 else 0.0
        lr = FO.lens_for(cam, T, W, T(k_px))
        F, K, Rm = FO.host_constants(cam, T, W, lr, fd, max_radius)
        assert K == T(k_px)
        top = min(float(K), float(Rm))
        target = rng.uniform(0.0, top, size=(H, W)).astype(T)
        below = np.zeros((H, W), bool)
        palette = [(v, bl) for v in (4.0, 8.0) if v < top for bl in (False, True)]
        if palette:
            pick, idx = rng.random((H, W)) < 0.4, rng.integers(len(palette), size=(H, W))
            for q, (val, bl) in enumerate(palette):
                sel = pick & (idx == q)
                target, below = np.where(sel, T(val), target), np.where(sel, bl, below)
        z = FO._plant_depth(cam, T, H, W, K, F, target, below)
        if k_px == 40:
            near = rng.random((H, W)) < 0.15                     # in front of the focus plane: up to the clamp
            z = np.where(near, (F * rng.uniform(0.02, 0.9, size=(H, W))).astype(T), z)
        cov = np.where(squares(0.3) | (rng.random((H, W)) < 0.05), 0.0, 1.0)
        albedo = rng.uniform(0.05, 1.0, size=(H, W, 3))
        nv = rng.normal(size=(H, W, 3))
        nv /= np.linalg.norm(nv, axis=2, keepdims=True)
        image = (albedo * rng.uniform(0.0, 2.0, size=(H, W, 1)) * rng.uniform(0.5, 1.5, size=(H, W, 3))).astype(T)
        feat = np.concatenate([albedo, nv * cov[..., None], np.zeros((H, W, 1)), cov[..., None]], axis=2).astype(T)
        feat[..., 6] = np.where(cov > 0, z, T(0))                # (cov is 0 or 1 here: depth*cov is the planted depth itself)
        if H * W >= 12:
            dead = squares(0.08) if min(H, W) >= 8 else np.zeros((H, W), bool)
            image[dead, 1] = np.nan
            for arr, ch, val in ((image, 1, np.nan), (feat, 7, np.inf), (feat, 4, -np.inf), (image, 0, np.inf), (image, 2, np.nan), (feat, 0, np.nan)):
                arr[int(rng.integers(H)), int(rng.integers(W)), ch] = val
        cases.append(dict(image=image, features=feat, cam=cam, params=dict(lens_radius=lr, focus_dist=fd, max_radius=max_radius, gamma=n % 2)))
    return cases


REGIMES = ["r4_at", "r4_below", "r4_above", "r8_at", "r8_below", "r8_above", "t_inside", "tap_skipped", "block_empty", "block_partial", "block_clipped", "a0_minus1", "a1_at_h",
           "block_sky_min"] + [f"block_clamp_{r}" for r in (9, 12, 16, 17, 24, 32)] + [f"lo_m{k}" for k in range(1, 9)]


def census(case, T):
    """which regimes one case reaches, counted on the witness alone (pixels, blocks or taps)"""
    T = np.dtype(T).type
    d = {}
    _, work = wide_aperture(case["image"], case["features"], case["cam"], T, details=d, **case["params"])
    R, valid = work["coc"][..., 0], d["valid"]
    h, w = work["lo_coc"].shape[:2]
    s = scale_of(case["params"]["max_radius"])
    out = dict.fromkeys(REGIMES, 0)
    with np.errstate(all="ignore"):
        for name, x in (("r4", T(4)), ("r8", T(8))):
            out[name + "_at"] = int((valid & (R == x)).sum())
            out[name + "_below"] = int((valid & (R < x) & (R >= x - T(NEAR))).sum())
            out[name + "_above"] = int((valid & (R > x) & (R <= x + T(NEAR))).sum())
        out["t_inside"] = int((valid & (d["t"] > 0) & (d["t"] < 1)).sum())
    out["tap_skipped"] = int(d["skipped"].sum())
    n, n_in = d["block_n"], d["block_in"]
    out["block_empty"] = int((n == 0).sum())
    out["block_partial"] = int(((n > 0) & (n < n_in)).sum())
    out["block_clipped"] = int((n_in < s * s).sum())
    H, W = valid.shape
    out["a0_minus1"] = int((valid & (d["a0"] == -1)[:, None]).sum() + (valid & (d["b0"] == -1)[None, :]).sum())
    out["a1_at_h"] = int((valid & (d["a0"] + 1 == h)[:, None]).sum() + (valid & (d["b0"] + 1 == w)[None, :]).sum())
    out["block_sky_min"] = int(((n > 0) & np.isinf(work["lo_coc"][..., 1])).sum())
    out[f"block_clamp_{case['params']['max_radius']}"] = int(((n > 0) & (d["block_clamp"] == n)).sum())
    lo_valid = ~np.isnan(work["lo_coc"][..., 1])
    for k in range(1, 9):
        out[f"lo_m{k}"] = int((lo_valid & d["lo_filt"] & (d["lo_m"] == k)).sum())
    return out
