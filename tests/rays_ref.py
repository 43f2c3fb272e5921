"""Ray queries (include/rtw_hip.h rtw_cast_rays_*): the witness and the ray populations of tests/test_rays_ref.py (CPU: a census of the
populations on the oracle alone) and tests/test_gpu_rays.py (the device against the oracle, on the bits).  A plain helper module: seeded,
no file fixtures beyond the golden scenes the suite already has.

The expected result of a ray is rtw_oracle.hit_world(scene, o, d, tmin, tmax_i) -- per ray, bounded by the ray's OWN tmax, in the numerics
mode that is current -- as (idx, rec[8]); rtw_oracle.hit_world_batch (unbounded) builds the populations that need a hit point or a root and
is the other side of the equivalence the kernel relies on (the bounded scan = the unbounded scan, then "miss if tmax < t").

The populations are built ONCE per (scene, precision), in binary64 and in the oracle's reference mode, then rounded to T: the rays are the
same in every numerics mode, directions are of unit length to one rounding.  Population letters are the issue's:
  a  primary rays of the scene's camera at 16 x 9 (pixel centres)
  b  bounce rays: origins the oracle's hit points of (a), directions random unit vectors, every fourth one grazing the surface it starts
     on (tangent, tilted inwards so that the sphere is left again after t ~ 5e-4): the tmin re-hit regime
  c  inside rays: two rays from inside each of up to 24 spheres (the largest, the negative radii, a spread of the rest); every third one
     with tmax = |r| / 2, which ends before the sphere is left
  d  limb rays: past the four largest spheres that are no ground, in the plane of the camera's view direction and "up", passing the
     centre c at the distance r (1 +- 2^-k), k = 4 .. 20 -- aimed at c + rho e, e the part of "up" across the view direction and rho the
     offset that makes the RAY (not the aim point) keep that distance: aimed at c + r (1 +- 2^-k) e itself, an origin at a finite distance
     sees every ray with k >= 8 hit.  They start on the camera's line of sight two radii in front of the centre: from the camera, ten
     units away, binary32 cannot tell the two sides apart beyond k = 16.  They fall on both sides of disc = 0
  e  population (a) with tmax set, in rotation over the rays that hit: the oracle's unbounded t, its two neighbours, tmin, tmin / 2, +inf
     (the rays that miss rotate over the last three)
  f  the directions of (a) scaled by 0.5, 1.001 and 2
  g  the origins of (a) moved along -d to |o| = 1e3, 1e6 and 1e12 (beyond every scene's mf_o_max: no stat or unit op exposes it)
  t  (the duplicate scene only) rays at the centre of every sphere from the camera and from the far side"""
import numpy as np

import rtw_oracle as O
from conftest import load_golden

TMIN = 1e-4                 # the reference's; converted to T once by both sides
W, H = 16, 9
TMAX_CHOICES = ("t", "below", "above", "tmin", "under_tmin", "inf")
LIMB_K = tuple(range(4, 21))
FAR = (1e3, 1e6, 1e12)
SCALES = (0.5, 1.001, 2.0)
SCENES = ("two", "random", "bubble", "dup", "big")
DUP_FIRST, DUP_SECOND, DUP_PAIR = 5, 20, (31, 32)
_cache = {}


def _cam64(cam):
    return {k: np.asarray(cam[k], np.float64) for k in ("origin", "lower_left_corner", "horizontal", "vertical")}


def dup_scene(T):
    """33 spheres of radius 0.3 on an 11 x 3 grid; sphere 20 is sphere 5 again and sphere 32 is sphere 31 again (across the block of 32)"""
    k = np.arange(33)
    cx, cy, cz, r = (k % 11 - 5.0), np.zeros(33), -(k // 11).astype(np.float64), np.full(33, 0.3)
    for a in (cx, cy, cz, r):
        a[DUP_SECOND] = a[DUP_FIRST]
        a[DUP_PAIR[1]] = a[DUP_PAIR[0]]
    rng = np.random.default_rng(33)
    alb = rng.uniform(0.1, 0.9, (33, 3))
    return dict(n=33, cx=cx.astype(T), cy=cy.astype(T), cz=cz.astype(T), r=r.astype(T), kind=np.zeros(33, np.int32), ar=alb[:, 0].astype(T),
                ag=alb[:, 1].astype(T), ab=alb[:, 2].astype(T), param=np.zeros(33, T))


def scene(name, T):
    """-> (flat scene of dtype T, camera as float64 arrays); computed once, read-only"""
    T = np.dtype(T).type
    key = ("scene", name, np.dtype(T).name)
    if key in _cache:
        return _cache[key]
    if name in ("two", "bubble"):
        g = load_golden("cfg1_2spheres_96x54_16spp_d4_f32" if name == "two" else "diel_bubble_96x54_8spp_d16_f32", numerics="reference")
        flat = {k: (np.asarray(v).astype(T) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in g["flat"].items()}
        cam = _cam64(g["cam"])
    elif name == "random":
        flat = O.scene_random_spheres(1, T)
        cam = _cam64(O.default_camera([13, 2, 3], [0, 0, 0], [0, 1, 0], 20, 16 / 9, 0.0, 10, np.float64))
    elif name == "dup":
        flat = dup_scene(T)
        cam = _cam64(O.default_camera([0, 3, 8], [0, 0, -1], [0, 1, 0], 40, 16 / 9, 0.0, 10, np.float64))
    elif name == "big":
        import big_scenes as BS
        flat = BS.scene(T)
        c = BS.cameras(T)[0]
        cam = _cam64({k: getattr(c, k) for k in ("origin", "lower_left_corner", "horizontal", "vertical")})
    else:
        raise ValueError(name)
    for v in flat.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cache[key] = (flat, cam)
    return _cache[key]


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def pack(o, d, tmax=None, T=np.float32):
    """origins, directions (binary64 or T) and tmax (None: +inf) -> rays [n, 8] of T, tag = the ray's number"""
    o, d = np.asarray(o), np.asarray(d)
    rays = np.zeros((o.shape[0], 8), T)
    rays[:, 0:3] = o
    rays[:, 3:6] = d
    rays[:, 6] = np.inf if tmax is None else tmax
    rays[:, 7] = np.arange(o.shape[0])
    return rays


def unbounded(flat, rays, T):
    """hit_world_batch with tmax = +inf -> (idx, t)"""
    return O.hit_world_batch(flat, np.ascontiguousarray(rays[:, 0:6]), TMIN, np.inf, T)


def expected(flat, rays, T):
    """The witness: per ray the oracle's hit_world bounded by the ray's own tmax, in the current numerics mode -> (idx [n] int32,
    rec [n, 8] of T: all +0 on a miss)."""
    T = np.dtype(T).type
    idx = np.empty(rays.shape[0], np.int32)
    rec = np.zeros((rays.shape[0], 8), T)
    for i, ray in enumerate(rays):
        k, r = O.hit_world(flat, ray[0:3], ray[3:6], TMIN, float(ray[6]), T)
        idx[i] = k
        if k >= 0:
            rec[i] = r
    return idx, rec


def _primary(cam):
    j, i = np.meshgrid(np.arange(W), np.arange(H))
    u, v = ((j.ravel() + 0.5) / W)[:, None], ((H - 1 - i.ravel() + 0.5) / H)[:, None]
    d = cam["lower_left_corner"] + u * cam["horizontal"] + v * cam["vertical"] - cam["origin"]
    return np.broadcast_to(cam["origin"], d.shape).copy(), _unit(d)


def _pick_inside(flat):
    r = np.abs(np.asarray(flat["r"], np.float64))
    n = int(flat["n"])
    order = list(np.argsort(-r)[:4]) + [k for k in range(n) if flat["r"][k] < 0][:4] + list(np.linspace(0, n - 1, 16).astype(int))
    seen, out = set(), []
    for k in order:
        if int(k) not in seen:
            seen.add(int(k))
            out.append(int(k))
    return out[:24]


def populations(name, T):
    """-> {letter: rays [n, 8] of T} and, under "meta", what the census needs (the tmax choice of every ray of (e), the k and the side
    of every ray of (d), the scale of every ray of (f), the distance of every ray of (g)); computed once, read-only"""
    T = np.dtype(T).type
    key = ("pop", name, np.dtype(T).name)
    if key in _cache:
        return _cache[key]
    flat, cam = scene(name, T)
    n = int(flat["n"])
    c64 = np.stack([np.asarray(flat[k], np.float64) for k in ("cx", "cy", "cz")], axis=1)
    r64 = np.asarray(flat["r"], np.float64)
    rng = np.random.default_rng(20 + SCENES.index(name))
    pops, meta = {}, {}
    prev = O.set_numerics("reference")
    try:
        # a
        o, d = _primary(cam)
        pops["a"] = pack(o, d, None, T)
        a_idx, a_t = unbounded(flat, pops["a"], T)
        # b: from the hit points of (a), as the oracle has them (in T)
        hit = np.nonzero(a_idx >= 0)[0]
        _, a_rec = expected(flat, pops["a"], T)
        bo = a_rec[hit, 1:4]
        bd = _unit(rng.normal(size=(hit.size, 3)))
        for m in range(0, hit.size, 4):
            s = int(a_idx[hit[m]])
            nrm = _unit(bo[m].astype(np.float64) - c64[s])
            tan = _unit(np.cross(nrm, [0.3, 0.5, 0.8]))
            bd[m] = _unit(tan - (2.5e-4 / abs(r64[s])) * nrm)
        pops["b"] = pack(bo, bd, None, T)
        # c
        co, cd, ct = [], [], []
        for m, s in enumerate(_pick_inside(flat)):
            for q in range(2):
                co.append(c64[s] + 0.3 * abs(r64[s]) * _unit(rng.normal(size=3)))
                cd.append(_unit(rng.normal(size=3)))
                ct.append(0.5 * abs(r64[s]) if (2 * m + q) % 3 == 2 else np.inf)
        pops["c"] = pack(np.array(co), np.array(cd), np.array(ct), T)
        # d
        big = [int(k) for k in np.argsort(-np.abs(r64)) if abs(r64[k]) < 100][:4]
        do, dd, dk, dside = [], [], [], []
        for s in big:
            view = _unit(c64[s] - cam["origin"])
            e = _unit(np.array([0.0, 1.0, 0.0]) - view[1] * view)
            for k in LIMB_K:
                for side in (-1, 1):
                    miss = abs(r64[s]) * (1.0 + side * 2.0 ** -k)            # how far from the centre the ray passes
                    dist = 2.0 * abs(r64[s])
                    start = c64[s] - dist * view
                    aim = c64[s] + miss * dist / np.sqrt(dist * dist - miss * miss) * e
                    do.append(start)
                    dd.append(_unit(aim - start))
                    dk.append(k)
                    dside.append(side)
        pops["d"] = pack(np.array(do), np.array(dd), None, T)
        meta["d_k"], meta["d_side"] = np.array(dk), np.array(dside)
        # e
        tmin_T = T(TMIN)
        tmax, choice = np.empty(a_idx.size, T), np.empty(a_idx.size, np.int32)
        nh = nm = 0
        for i in range(a_idx.size):
            if a_idx[i] >= 0:
                ch, nh = nh % 6, nh + 1
            else:
                ch, nm = 3 + nm % 3, nm + 1
            choice[i] = ch
            tmax[i] = (a_t[i], np.nextafter(a_t[i], T(-np.inf)), np.nextafter(a_t[i], T(np.inf)), tmin_T, tmin_T / T(2), T(np.inf))[ch]
        pops["e"] = pack(o, d, tmax, T)
        meta["e_choice"] = choice
        # f
        dT = pops["a"][:, 3:6].astype(np.float64)
        pops["f"] = np.concatenate([pack(o, dT * s, None, T) for s in SCALES])
        meta["f_scale"] = np.repeat(SCALES, o.shape[0])
        # g
        go = []
        for dist in FAR:
            back = o - d * dist
            go.append(back * (dist / np.linalg.norm(back, axis=1, keepdims=True)))        # |o| = dist
        pops["g"] = np.concatenate([pack(x, d, None, T) for x in go])
        meta["g_dist"] = np.repeat(FAR, o.shape[0])
        if name == "dup":
            to = np.concatenate([np.broadcast_to(cam["origin"], (n, 3)), 2.0 * c64 - cam["origin"]])
            td = _unit(np.concatenate([c64, c64]) - to)
            pops["t"] = pack(to, td, None, T)
    finally:
        O.set_numerics(prev)
    for k in pops:
        pops[k][:, 7] = np.arange(pops[k].shape[0])
        pops[k].setflags(write=False)
    pops["meta"] = meta
    _cache[key] = pops
    return pops


def letters(name):
    return [k for k in populations(name, np.float32) if k != "meta"]


def reference(name, letter, T):
    """the witness's (idx, rec) of a population in the current numerics mode; computed once, read-only"""
    key = ("ref", name, letter, np.dtype(T).name, O._default_numerics)
    if key not in _cache:
        flat, _ = scene(name, T)
        idx, rec = expected(flat, populations(name, T)[letter], T)
        idx.setflags(write=False)
        rec.setflags(write=False)
        _cache[key] = (idx, rec)
    return _cache[key]


def all_rays(name, T, which=None):
    """the populations of a scene one behind the other -> (rays [n, 8], idx, rec, {letter: slice}); `which`: the letters (None: all)"""
    parts, idxs, recs, where, at = [], [], [], {}, 0
    for k in (which or letters(name)):
        rays = populations(name, T)[k]
        i, r = reference(name, k, T)
        parts.append(rays)
        idxs.append(i)
        recs.append(r)
        where[k] = slice(at, at + rays.shape[0])
        at += rays.shape[0]
    return np.concatenate(parts), np.concatenate(idxs), np.concatenate(recs), where


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)
