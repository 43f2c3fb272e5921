"""Radiance queries (include/rtw_hip.h rtw_trace_rays_*): the witness and the ray lists of tests/test_trace_rays_ref.py (CPU: the witness
written twice, and a census of the lists on the oracle alone) and tests/test_gpu_trace_rays.py (the device against the witness, on the
bits).  A plain helper module: seeded, scenes and populations are those of tests/rays_ref.py, read-only.

Sample s of ray i is ray_color(scene, o_i, d_i, max_depth) on the fresh stream rng_stream(seed, first_stream + i, first_sample + s); the
result of a ray is, per channel, the exact 64.64 sum of its spp radiances rounded once (rtw_oracle.fx_sum) and divided by spp, all three
NaN when a sample was NaN, infinite or >= 2^31.

The witness is written twice:
  (A) rtw_oracle.ray_color(..., PRODUCT_FORWARD) per ray, sample and depth -- the oracle's own loop;
  (B) the loop restated from the oracle's unit calls hit_world, scatter and skycolor, the product formed front to back, walked ONCE per
      sample up to MAX_SCANS segments: the radiance under max_depth D is thr * sky where the path's miss is among its first D scans and
      0 where it is not (a path draws nothing that depends on D, so the longer walk has the shorter one as its prefix).  This form also
      counts the scans (what rtw_stats() reports as segments) and takes the census.
Sample radiances are kept per (scene, precision, numerics mode, seed, first_stream, first_sample) for MAX_SPP samples: spp = 1 and 2 are
prefixes of spp = 7."""
import numpy as np

import rtw_oracle as O
import rays_ref as RR

TMIN = 1e-4
SPPS = (1, 2, 7)
DEPTHS = (1, 2, 16, 50)
MAX_SPP = max(SPPS)
MAX_SCANS = max(DEPTHS)
SMALL_SCENES = ("two", "random", "bubble", "dup")
SEED = 11
_cache = {}


def rays_of(name, T):
    """the list of a scene: every second primary ray, every second bounce ray, every inside ray (populations a, b, c of rays_ref) ->
    (rays [n, 8] of T, {letter: slice}); about 200 rays; read-only"""
    key = ("rays", name, np.dtype(T).name)
    if key not in _cache:
        pops = RR.populations(name, T)
        parts, where, at = [], {}, 0
        for k, step in (("a", 2), ("b", 2), ("c", 1)):
            p = pops[k][::step]
            parts.append(p)
            where[k] = slice(at, at + p.shape[0])
            at += p.shape[0]
        rays = np.concatenate(parts)
        rays.setflags(write=False)
        _cache[key] = (rays, where)
    return _cache[key]


def big_rays(T):
    """64 rays of the scene the global-memory instances take: primary and inside rays"""
    pops = RR.populations("big", T)
    rays = np.concatenate([pops["a"][::3][:44], pops["c"][:20]])
    rays.setflags(write=False)
    return rays


def edge_rays(T):
    """1000 rays of the 485-sphere scene: all its populations, the scaled directions and far origins among them (every finite ray has a
    defined result)"""
    key = ("edge", np.dtype(T).name)
    if key not in _cache:
        pops = RR.populations("random", T)
        rays = np.concatenate([pops[k] for k in ("a", "b", "c", "d", "f", "g")])[:1000].copy()
        assert rays.shape[0] == 1000
        rays.setflags(write=False)
        _cache[key] = rays
    return _cache[key]


# ---- (A) ------------------------------------------------------------------------------------------------------------------------------
def sample_radiances(flat, rays, T, depth, spp, seed=SEED, first_stream=0, first_sample=0):
    """-> [n, spp, 3] binary64: the oracle's ray_color of every sample, in the numerics mode that is current"""
    out = np.empty((rays.shape[0], spp, 3), np.float64)
    for i, ray in enumerate(rays):
        for s in range(spp):
            st = O.rng_stream(seed, first_stream + i, first_sample + s)
            out[i, s], _ = O.ray_color(flat, ray[0:3], ray[3:6], depth, st, O.PRODUCT_FORWARD, T)
    return out


def resolve(rad):
    """sample radiances [n, spp, 3] -> the result [n, 3]: fx_sum per ray and channel, / spp, the poison rule"""
    n, spp, _ = rad.shape
    out = np.empty((n, 3), np.float64)
    for i in range(n):
        bad = 0
        for c in range(3):
            v, b = O.fx_sum(rad[i, :, c])
            out[i, c] = v / float(spp)
            bad += b
        if bad:
            out[i, :] = np.nan
    return out


def radiances_a(name, T, depth, **kw):
    """(A) of a scene's list for MAX_SPP samples at `depth`; computed once per numerics mode, read-only"""
    key = ("A", name, np.dtype(T).name, depth, O._default_numerics, tuple(sorted(kw.items())))
    if key not in _cache:
        flat = RR.scene(name, T)[0]
        rays = big_rays(T) if name == "big" else rays_of(name, T)[0]
        rad = sample_radiances(flat, rays, T, depth, MAX_SPP, **kw)
        rad.setflags(write=False)
        _cache[key] = rad
    return _cache[key]


def expected(name, T, depth, spp, **kw):
    """the witness (A) of a scene's list -> [n, 3] binary64"""
    return resolve(radiances_a(name, T, depth, **kw)[:, :spp])


# ---- (B) ------------------------------------------------------------------------------------------------------------------------------
def _draws(before, after, limit=3000):
    st = np.array(before, np.uint64)
    for k in range(limit + 1):
        if st[0] == after[0] and st[1] == after[1]:
            return k
        O.rng_next(st)
    raise AssertionError("the stream did not reach the state scatter left")


def walk(flat, o, d, state, T, max_scans=MAX_SCANS):
    """One sample, restated from the unit calls -> dict: n_scans (scans until the miss, max_scans where there is none), missed, rad (thr *
    sky at the miss), and per scattering segment its kind, its draws and, for a dielectric, whether the ray went through."""
    T = np.dtype(T).type
    thr = np.ones(3, np.float64)
    o, d = np.asarray(o, T), np.asarray(d, T)
    state = np.array(state, np.uint64)
    kinds, draws, through = [], [], []
    for k in range(max_scans):
        idx, rec = O.hit_world(flat, o, d, TMIN, np.inf, T)
        if idx < 0:
            return dict(n_scans=k + 1, missed=True, rad=thr * O.skycolor(d, T), kinds=kinds, draws=draws, through=through)
        kind = int(flat["kind"][idx])
        out, st2 = O.scatter(kind, (flat["ar"][idx], flat["ag"][idx], flat["ab"][idx]), flat["param"][idx], d, rec, state, T)
        kinds.append(kind)
        draws.append(_draws(state, st2))
        through.append(kind == 2 and float(np.dot(out[3:6].astype(np.float64), rec[4:7].astype(np.float64))) < 0.0)
        thr = thr * out[6:9].astype(np.float64)               # ((1 * att1) * att2) ...: front to back, one rounding each
        o, d, state = out[0:3].copy(), out[3:6].copy(), st2
    return dict(n_scans=max_scans, missed=False, rad=np.zeros(3), kinds=kinds, draws=draws, through=through)


def walks(name, T, seed=SEED):
    """(B): every sample of a scene's list walked once -> [n][MAX_SPP] dicts; computed once per numerics mode"""
    key = ("B", name, np.dtype(T).name, O._default_numerics, seed)
    if key not in _cache:
        flat = RR.scene(name, T)[0]
        rays = rays_of(name, T)[0]
        _cache[key] = [[walk(flat, ray[0:3], ray[3:6], O.rng_stream(seed, i, s), T) for s in range(MAX_SPP)] for i, ray in enumerate(rays)]
    return _cache[key]


def radiances_b(name, T, depth):
    """(B)'s sample radiances under max_depth = depth -> [n, MAX_SPP, 3]"""
    W = walks(name, T)
    out = np.zeros((len(W), MAX_SPP, 3), np.float64)
    for i, row in enumerate(W):
        for s, w in enumerate(row):
            if w["missed"] and w["n_scans"] <= depth:
                out[i, s] = w["rad"]
    return out


def segments_b(name, T, depth, spp):
    """(B)'s count of scans with a live ray: what rtw_stats() reports as segments"""
    return sum(min(w["n_scans"], depth) for row in walks(name, T) for w in row[:spp])


def long_path_list(T):
    """the bubble scene: -> (the ray of its list whose samples scan most -- it starts inside the glass, and a sample of it is cut off at
    depth 50 --, rays from high above the scene that point upwards and miss at once [>= 100, 8])"""
    key = ("long", np.dtype(T).name)
    if key not in _cache:
        flat = RR.scene("bubble", T)[0]
        rays = rays_of("bubble", T)[0]
        prev = O.set_numerics("reference")
        try:
            W = walks("bubble", T)
            scans = [sum(w["n_scans"] for w in row) for row in W]
            i = int(np.argmax(scans))
            assert any(not w["missed"] for w in W[i]), "no sample of the longest ray runs out of depth 50"
            rng = np.random.default_rng(50)
            d = rng.normal(size=(160, 3))
            d[:, 1] = np.abs(d[:, 1]) + 0.5
            up = RR.pack(np.tile([0.0, 30.0, 0.0], (160, 1)), d / np.linalg.norm(d, axis=1, keepdims=True), None, T)
            idx, _ = RR.unbounded(flat, up, T)
        finally:
            O.set_numerics(prev)
        misses = up[idx < 0]
        misses.setflags(write=False)
        _cache[key] = (rays[i].copy(), misses)
    return _cache[key]


def same_words(a, b):
    """binary64 arrays equal on the bits, NaN matched as NaN"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


def sky(rays, T):
    """sky(d) of every ray -> [n, 3] binary64"""
    return np.array([O.skycolor(r[3:6], T) for r in rays])
