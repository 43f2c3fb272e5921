"""The material parameter space of the shading path (a plain helper module): a scene whose spheres span refraction indices on both
sides of 1, bubbles, fuzz 0 .. 3 and albedos 0 .. 1.5; a census of what the oracle's paths do in it; and the inputs of one bounce that sit
ON the decisions of scatter -- the total-internal-reflection comparison `ratio * sin_t > 1`, the Schlick comparison `reflectance > u`, the
`cos_t` clamp, Lambertian `near_zero`, fuzz 0.  Every edge input is found by bisection on the CPU oracle alone: the two ADJACENT
representable inputs between which the oracle's answer changes.  Nothing of the product is used.

    sweep_scene(T, extra)      the scene and its camera
    census(flat, cam, ...)     scatter events of the first sample of every pixel, by sphere, face and branch
    tir_pairs / schlick_pairs / clamp_inputs / near_zero_inputs / metal_inputs      one-bounce inputs for unit ops 1 - 4
    shade_*                    the same decisions for unit op 26: a one-sphere scene and rays whose hit the oracle puts on either side
Results are cached per precision: the tests share one computation and must leave it unchanged."""
from collections import namedtuple

import numpy as np

import rtw_oracle as O

LAMBERTIAN, METAL, DIELECTRIC = 0, 1, 2
PRECISIONS = [np.float32, np.float64]
N_BASE = 18
GROUND = 0
DIELECTRICS = list(range(1, 11))            # the eight solid spheres, then the two bubbles
METALS = list(range(11, 15))
LAMBERTIANS = list(range(15, 18))
IRS = [1.0, 1.05, 1.33, 2.417, 0.75, 1 / 1.5, 4.0, 1.5]
FUZZ = [0.0, 0.25, 1.0, 3.0]
#: (ir, front face) of the total-internal-reflection thresholds: the ratio is above 1 on a back face of ir > 1 and on a front face of ir < 1
TIR_CASES = [(1.5, False), (0.75, True), (2.417, False), (1 / 1.5, True)]
SCHLICK_CASES = [(ir, front) for ir, _ in TIR_CASES for front in (True, False)]
#: the Schlick ties: every case at two uniforms (schlick_pairs)
SCHLICK_ITEMS = [(ir, front, which) for ir, front in SCHLICK_CASES for which in ("mid", "low")]

_cache = {}


def _t(T):
    return np.dtype(T).type


def _readonly(flat):
    for v in flat.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return flat


def sweep_scene(T, extra=0):
    """-> (flat scene dict, camera dict).  18 spheres in the caller's order: the ground, eight dielectrics of IRS, two bubbles (negative
    radius) inside the second and the fifth, four metals of FUZZ, three Lambertians of albedo 0, 1 and (1.5, 0.25, 2^-20).  `extra` appends
    that many small Lambertians (radii 0.07 + 0.013 k, no power of two) in front of the rest: with 24 the scene spans two blocks of 32."""
    T = _t(T)
    key = ("scene", np.dtype(T).name, extra)
    if key in _cache:
        return _cache[key]
    rows = [((0.0, -1000.0, 0.0), 1000.0, LAMBERTIAN, (0.5, 0.5, 0.5), 0.0)]
    for k, ir in enumerate(IRS):
        rows.append(((-3.5 + k, 0.45, 0.0), 0.45, DIELECTRIC, (1.0, 1.0, 1.0), ir))
    rows.append(((-2.5, 0.45, 0.0), -0.35, DIELECTRIC, (1.0, 1.0, 1.0), 1.33))
    rows.append(((0.5, 0.45, 0.0), -0.30, DIELECTRIC, (1.0, 1.0, 1.0), 0.75))
    for k, fz in enumerate(FUZZ):
        rows.append(((-3.0 + 2 * k, 0.4, -1.2), 0.4, METAL, (0.9, 0.8, 0.7), fz))
    for k, alb in enumerate([(0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1.5, 0.25, 2.0 ** -20)]):
        rows.append(((-2.0 + 2 * k, 0.3, 1.0), 0.3, LAMBERTIAN, alb, 0.0))
    assert len(rows) == N_BASE
    for k in range(extra):
        r = 0.07 + 0.013 * k
        rows.append(((-3.45 + 0.3 * k, r, 2.2 + 0.45 * (k % 3)), r, LAMBERTIAN, (0.2 + 0.03 * k, 0.6, 0.9 - 0.03 * k), 0.0))
    c = np.array([r[0] for r in rows])
    alb = np.array([r[3] for r in rows])
    flat = dict(n=len(rows), cx=c[:, 0].astype(T), cy=c[:, 1].astype(T), cz=c[:, 2].astype(T), r=np.array([r[1] for r in rows]).astype(T),
                kind=np.array([r[2] for r in rows], np.int32), ar=alb[:, 0].astype(T), ag=alb[:, 1].astype(T), ab=alb[:, 2].astype(T),
                param=np.array([r[4] for r in rows]).astype(T))
    cam = O.default_camera((0, 2.2, 6.5), (0, 0.3, 0), (0, 1, 0), 38, 16 / 9, 0.1, 6.5, T)
    _cache[key] = (_readonly(flat), cam)
    return _cache[key]


def in_front_of_a_field(T, n_field=1600, seed=7):
    """the sweep's 18 spheres in front of a big_scenes-style field: n_field small spheres of all three materials on the ground behind and
    beside them (z < -2.5 or |x| > 4.6), so that the scene leaves the LDS scene copy.  -> (flat, cam)"""
    T = _t(T)
    key = ("field", np.dtype(T).name, n_field, seed)
    if key in _cache:
        return _cache[key]
    base, cam = sweep_scene(T)
    rng = np.random.default_rng(seed)
    x, z = np.empty(n_field), np.empty(n_field)
    for k in range(n_field):
        while True:
            x[k], z[k] = rng.uniform(-9, 9), rng.uniform(-12, 1.5)
            if z[k] < -2.5 or abs(x[k]) > 4.6:
                break
    r = rng.uniform(0.05, 0.25, n_field)
    kind = rng.integers(0, 3, n_field).astype(np.int32)
    alb = rng.uniform(0.1, 0.9, (n_field, 3))
    param = np.where(kind == METAL, rng.uniform(0, 0.5, n_field), np.where(kind == DIELECTRIC, rng.choice([1.5, 1.33, 0.9, 2.0], n_field), 0.0))
    cols = dict(cx=x, cy=r, cz=z, r=r, ar=alb[:, 0], ag=alb[:, 1], ab=alb[:, 2], param=param)
    flat = {k: np.concatenate([base[k], cols[k].astype(T)]) for k in cols}
    flat["kind"] = np.concatenate([base["kind"], kind])
    flat["n"] = N_BASE + n_field
    _cache[key] = (_readonly(flat), cam)
    return _cache[key]


# ---- what one scatter did, by the oracle --------------------------------------------------------------------------------------------------
def rec8(n, front, T, p=(0.0, 0.0, 0.0), t=1.0):
    """the hit record the oracle's scatter takes: t, p[3], n[3], front"""
    return np.array([t, *p, *n, 1.0 if front else 0.0], dtype=T)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def classify(kind, albedo, param, d, rec, state, T):
    """-> (branch, out9, state after).  Dielectric: 'tir' (the state did not advance), 'schlick' (the direction is reflect(d, n)),
    'refract'.  Lambertian: 'degenerate' (near_zero: the direction is the normal, as is) or 'ball'.  Metal: 'ball'."""
    state = np.array(state, np.uint64)
    out, s1 = O.scatter(kind, albedo, param, d, rec, state, T)
    if kind == DIELECTRIC:
        if np.array_equal(s1, state):
            return "tir", out, s1
        if _same(out[3:6], O.reflect(d, rec[4:7], T)):
            return "schlick", out, s1
        return "refract", out, s1
    if kind == LAMBERTIAN and _same(out[3:6], np.asarray(rec[4:7], dtype=T)):
        return "degenerate", out, s1
    return "ball", out, s1


def census(flat, cam, T, W, H, depth, seed=1):
    """The first sample of every pixel (chunk 0: centred, no jitter) followed through the oracle's unit calls.  -> dict with
    'tir' / 'schlick' / 'refract': int [n, 2] (sphere, face: 0 back, 1 front) and 'ball': int [n]"""
    T = _t(T)
    n = int(flat["n"])
    out = {k: np.zeros((n, 2), np.int64) for k in ("tir", "schlick", "refract")}
    out["ball"] = np.zeros(n, np.int64)
    alb = np.stack([flat["ar"], flat["ag"], flat["ab"]], 1)
    for j in range(1, W + 1):
        for i in range(1, H + 1):
            st = O.rng_stream(seed, (j - 1) * H + (i - 1), 0)
            ray, st = O.get_ray(cam, T(j / W), T((H - i) / H), st, T)
            o, d = ray[:3], ray[3:]
            for _ in range(depth):
                idx, rec = O.hit_world(flat, o, d, 1e-4, np.inf, T)
                if idx < 0:
                    break
                kind = int(flat["kind"][idx])
                branch, sc, st = classify(kind, alb[idx], flat["param"][idx], d, rec, st, T)
                if kind == DIELECTRIC:
                    out[branch][idx, int(rec[7] != 0)] += 1
                else:
                    out["ball"][idx] += 1
                o, d = sc[:3], sc[3:6]
    return out


def census_cached(T, extra=0, W=64, H=36, depth=16):
    key = ("census", np.dtype(T).name, extra, W, H, depth)
    if key not in _cache:
        flat, cam = sweep_scene(T, extra)
        _cache[key] = census(flat, cam, T, W, H, depth)
    return _cache[key]


# ---- bisection over the representable values of T ----------------------------------------------------------------------------------------
def _uint(T):
    return (np.uint64, 64) if np.dtype(T) == np.float64 else (np.uint32, 32)


def to_ordinal(x, T):
    """a value of T -> an integer that grows with it, neighbours 1 apart"""
    U, nb = _uint(T)
    b = int(np.array(x, dtype=T).view(U))
    mag = b & ((1 << (nb - 1)) - 1)
    return -mag if b >> (nb - 1) else mag


def from_ordinal(k, T):
    U, nb = _uint(T)
    return _t(T)(np.array(abs(k) | ((1 << (nb - 1)) if k < 0 else 0), dtype=U).view(T))


def bisect_flip(pred, lo, hi, T):
    """pred(lo) != pred(hi) -> (a, b): adjacent values of T between them with pred(a) == pred(lo) and pred(b) == pred(hi)"""
    a, b = to_ordinal(lo, T), to_ordinal(hi, T)
    pa, pb = pred(from_ordinal(a, T)), pred(from_ordinal(b, T))
    assert pa != pb and a < b
    while b - a > 1:
        m = (a + b) // 2
        if pred(from_ordinal(m, T)) == pa:
            a = m
        else:
            b = m
    return from_ordinal(a, T), from_ordinal(b, T)


# ---- one-bounce inputs (unit ops 1 - 4) ---------------------------------------------------------------------------------------------------
#: one input of scatter: material, incoming direction, hit normal and face, RNG state; `what` names the decision it sits at
Bounce = namedtuple("Bounce", "what kind albedo param d n front state")
UP = (0.0, 1.0, 0.0)
WHITE = (1.0, 1.0, 1.0)


def ratio_of(ir, front, T):
    """the refraction ratio scatter uses (src/material.jl:42-43), in T"""
    T = _t(T)
    return T(1) / T(ir) if front else T(ir)


def state_with_uniform(u, T):
    """a generator state whose NEXT uniform of type T is the multiple of 2^-23 / 2^-52 nearest to u: the uniform is made of the low 23 / 52
    bits of x + y (src/rand.jl:5-13), so y carries high bits only and x the wanted ones"""
    bits = 52 if np.dtype(T) == np.float64 else 23
    k = min(max(int(round(float(u) * 2 ** bits)), 0), 2 ** bits - 1)
    st = np.array([k | (0x5A5 << 52), 0x9E3779B97 << 28 & ~((1 << 52) - 1)], dtype=np.uint64)
    got = O.rng_float(st.copy(), T)
    assert float(got) == k / 2 ** bits, (got, k)
    return st


def grazing(s, T):
    """d = (s, -sqrt(1 - s s), 0) in T: against the normal (0, 1, 0) the cosine is exactly -d.y and the sine close to s"""
    T = _t(T)
    s = T(s)
    return np.array([s, -np.sqrt(T(1) - s * s), T(0)], dtype=T)


def falling(c, T):
    """d = (sqrt(1 - c c), -c, 0) in T: against the normal (0, 1, 0) the cosine is exactly c"""
    T = _t(T)
    c = T(c)
    return np.array([np.sqrt(T(1) - c * c), -c, T(0)], dtype=T)


def _dielectric(what, ir, d, front, state, T, n=UP):
    return Bounce(what, DIELECTRIC, WHITE, _t(T)(ir), np.asarray(d, dtype=T), np.asarray(n, dtype=T), front, np.array(state, np.uint64))


def branch_of(b, T):
    return classify(b.kind, b.albedo, b.param, b.d, rec8(b.n, b.front, T), b.state, T)[0]


def tir_pairs(T):
    """per (ir, face) of TIR_CASES: (below, above) -- two bounces whose s are neighbours in T; `below` draws a uniform, `above` reflects
    without one.  The state's first uniform is 0.75: above Schlick's reflectance at the critical angle, so `below` refracts."""
    T = _t(T)
    key = ("tir", np.dtype(T).name)
    if key not in _cache:
        state = state_with_uniform(0.75, T)
        out = []
        for ir, front in TIR_CASES:
            mk = lambda s: _dielectric(f"tir ir={ir:.4g} {'front' if front else 'back'}", ir, grazing(s, T), front, state, T)
            a, b = bisect_flip(lambda s: branch_of(mk(s), T) == "tir", T(0.05), T(0.999), T)
            out.append((mk(a), mk(b)))
        _cache[key] = out
    return _cache[key]


def schlick_pairs(T):
    """per (ir, face, which) of SCHLICK_ITEMS: (reflects, refracts, u) -- two bounces whose cosines are neighbours in T, below the critical
    angle, and the uniform u their state yields: reflectance(cos) > u for the first and not for the second.  'mid': u half way between
    Schlick's r0 and the reflectance just inside the critical angle (a range of a few hundred ulps for ir = 2.417 from inside).  'low':
    the first uniform above r0 -- there the reflectance is r0 plus a few of its ulps and stays on one value over thousands of
    neighbouring cosines, so an r0 that is one ulp off moves the flip far away from the pair."""
    T = _t(T)
    key = ("schlick", np.dtype(T).name)
    if key not in _cache:
        bits = 52 if np.dtype(T) == np.float64 else 23
        out = []
        for ir, front, which in SCHLICK_ITEMS:
            ratio = ratio_of(ir, front, T)
            c0 = schlick_start(ratio, T)
            r_hi, r_lo = float(O.reflectance(c0, ratio, T)), float(O.reflectance(T(1), ratio, T))
            assert r_hi > r_lo
            state = state_with_uniform(0.5 * (r_hi + r_lo) if which == "mid" else (np.floor(r_lo * 2 ** bits) + 1) / 2 ** bits, T)
            u = O.rng_float(state.copy(), T)
            assert r_lo < float(u) < r_hi, (ir, front, which, r_lo, float(u), r_hi)
            mk = lambda c: _dielectric(f"schlick ir={ir:.4g} {'front' if front else 'back'} u {which}", ir, falling(c, T), front, state, T)
            a, b = bisect_flip(lambda c: branch_of(mk(c), T) == "schlick", c0, T(1), T)
            out.append((mk(a), mk(b), u))
        _cache[key] = out
    return _cache[key]


def schlick_start(ratio, T):
    """a cosine just inside the critical angle of `ratio` (1e-3 for a ratio that has none)"""
    return _t(T)(np.sqrt(max(0.0, 1.0 - 1.0 / float(ratio) ** 2)) + 1e-3)


def clamp_inputs(T):
    """per (ir, face) of SCHLICK_CASES, against a normal of full mantissas: d = -n (cosine 1 up to rounding), d = -(1 + 2^-10) n (-d.n > 1:
    only the clamp keeps 1 - cos^2 from going negative) and, against (0, 1, 0), d = (1, 0, 0) (cosine 0, sine 1)"""
    T = _t(T)
    key = ("clamp", np.dtype(T).name)
    if key not in _cache:
        n = np.array([0.36, 0.48, 0.8], dtype=T)
        n = (n * (T(1) / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))).astype(T)
        state = state_with_uniform(0.5, T)
        out = []
        for ir, front in SCHLICK_CASES:
            face = "front" if front else "back"
            out.append(_dielectric(f"head-on ir={ir:.4g} {face}", ir, -n, front, state, T, n))
            out.append(_dielectric(f"clamped ir={ir:.4g} {face}", ir, (-(T(1) + T(2.0 ** -10)) * n).astype(T), front, state, T, n))
            out.append(_dielectric(f"perpendicular ir={ir:.4g} {face}", ir, (1.0, 0.0, 0.0), front, state, T))
        _cache[key] = out
    return _cache[key]


def ball_sample(state, T):
    """src/rand.jl:15-29 restated: the unit vector a Lambertian / Metal scatter draws from `state` -> (u [3] of T, state after).
    random_between(-1, 1) = trand * 2 - 1 is exact; a trial is accepted at len2 <= 1; u = (1 / sqrt(len2)) * p, every step in T."""
    T = _t(T)
    st = np.array(state, np.uint64)
    while True:
        p = np.array([O.rng_float(st, T) * T(2) + T(-1) for _ in range(3)], dtype=T)
        len2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
        if len2 <= T(1):
            return ((T(1) / np.sqrt(len2)) * p).astype(T), st


def _lambertian(what, n, state, T, d=(0.0, -1.0, 0.0)):
    return Bounce(what, LAMBERTIAN, (0.5, 0.25, 0.75), _t(T)(0), np.asarray(d, dtype=T), np.asarray(n, dtype=T), True, np.array(state, np.uint64))


def near_zero_inputs(T):
    """-> (exact, pairs): `exact` has n = -u, so n + u is exactly zero and the direction comes back as n, un-normalised; every pair is
    (degenerate, ball): n = -u + e along one axis, the two values of that component of n neighbours in T, |n + u|^2 on either side of
    1e-5.  Three states, one axis each."""
    T = _t(T)
    key = ("near_zero", np.dtype(T).name)
    if key not in _cache:
        exact, pairs = [], []
        for axis, seed in enumerate((21, 22, 23)):
            state = O.rng_stream(seed, 5, 0)
            u, _ = ball_sample(state, T)
            exact.append(_lambertian("n = -u", -u, state, T))

            def mk(x, axis=axis, u=u, state=state):
                n = (-u).copy()
                n[axis] = x
                return _lambertian(f"|n + u|^2 at 1e-5, axis {axis}", n, state, T)
            a, b = bisect_flip(lambda x: branch_of(mk(x), T) == "degenerate", -u[axis], -u[axis] + T(0.0625), T)
            pairs.append((mk(a), mk(b)))
        _cache[key] = (exact, pairs)
    return _cache[key]


def unit_dirs(rng, n, T):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(T)


def metal_inputs(T, per_fuzz=6):
    """Metal bounces of fuzz 0, 1 and 5 on random directions (the normal faces the ray)"""
    T = _t(T)
    key = ("metal", np.dtype(T).name, per_fuzz)
    if key not in _cache:
        rng = np.random.default_rng(31)
        out = []
        for fz in (0.0, 1.0, 5.0):
            d, n = unit_dirs(rng, per_fuzz, T), unit_dirs(rng, per_fuzz, T)
            for k in range(per_fuzz):
                nk = -n[k] if float(np.dot(d[k].astype(np.float64), n[k].astype(np.float64))) > 0 else n[k]
                out.append(Bounce(f"metal fuzz={fz:g}", METAL, (0.9, 0.8, 0.7), T(fz), d[k], nk, True, O.rng_stream(41, k, int(fz))))
        _cache[key] = out
    return _cache[key]


def normalize_t(v, T):
    """StaticArrays' normalize restated in T: (1 / sqrt((x x + y y) + z z)) * v"""
    T = _t(T)
    v = np.asarray(v, dtype=T)
    return ((T(1) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])) * v).astype(T)


def all_bounces(T):
    """every one-bounce input of the builders, in one list"""
    out = [b for p in tir_pairs(T) for b in p] + [b for p in schlick_pairs(T) for b in p[:2]] + list(clamp_inputs(T))
    exact, pairs = near_zero_inputs(T)
    return out + list(exact) + [b for p in pairs for b in p] + list(metal_inputs(T))


# ---- the same decisions behind a hit (unit op 26) -----------------------------------------------------------------------------------------
#: one item of op 26: a one-sphere scene, a ray and a state; `branch` is what the oracle's hit_world + scatter make of it
Shade = namedtuple("Shade", "what flat o d state branch")
SHADE_C, SHADE_R = (0.25, 0.45, -0.5), 0.45          # centre and radius (no power of two: the normal's division rounds)


def one_sphere(kind, albedo, param, T, r=SHADE_R):
    T = _t(T)
    f = lambda v: np.array([v], dtype=T)
    return _readonly(dict(n=1, cx=f(SHADE_C[0]), cy=f(SHADE_C[1]), cz=f(SHADE_C[2]), r=f(r), kind=np.array([kind], np.int32),
                          ar=f(albedo[0]), ag=f(albedo[1]), ab=f(albedo[2]), param=f(param)))


def aimed_ray(d, n, front, T):
    """A ray of direction d that meets the sphere (SHADE_C, SHADE_R) where the face-forwarded normal is about n: from outside towards
    c + r n for a front face, from the middle of its chord inside the sphere towards c - r n for a back face.  The hit's own d and n are
    what the solver makes of it."""
    T = _t(T)
    d64, n64 = np.asarray(d, np.float64), np.asarray(n, np.float64)
    p = np.array(SHADE_C) + SHADE_R * (n64 if front else -n64)
    o = p - (0.75 if front else SHADE_R * -float(np.dot(d64, n64))) * d64
    return o.astype(T), np.asarray(d, dtype=T)


def shade_branch(flat, o, d, state, T):
    """what the oracle makes of one item: hit_world, then scatter on its hit record -> (branch or 'miss', idx, out9, state after, front)"""
    idx, rec = O.hit_world(flat, o, d, 1e-4, np.inf, T)
    if idx < 0:
        return "miss", idx, None, np.array(state, np.uint64), None
    alb = [flat[k][idx] for k in ("ar", "ag", "ab")]
    branch, out, s1 = classify(int(flat["kind"][idx]), alb, flat["param"][idx], d, rec, state, T)
    return branch, idx, out, s1, bool(rec[7])


def _shade(what, flat, d, n, front, state, T):
    o, dd = aimed_ray(d, n, front, T)
    branch, _, _, _, face = shade_branch(flat, o, dd, state, T)
    assert branch != "miss" and face == front, (what, branch, face)
    return Shade(what, flat, o, dd, np.array(state, np.uint64), branch)


def shade_tir_pairs(T):
    """per (ir, face) of TIR_CASES: two items whose s are neighbours in T, the first draws, the second reflects without a draw"""
    T = _t(T)
    key = ("shade_tir", np.dtype(T).name)
    if key not in _cache:
        state = state_with_uniform(0.75, T)
        out = []
        for ir, front in TIR_CASES:
            flat = one_sphere(DIELECTRIC, WHITE, ir, T)
            mk = lambda s: _shade(f"tir ir={ir:.4g} {'front' if front else 'back'}", flat, grazing(s, T), UP, front, state, T)
            a, b = bisect_flip(lambda s: mk(s).branch == "tir", T(0.05), T(0.999), T)
            out.append((mk(a), mk(b)))
        _cache[key] = out
    return _cache[key]


def shade_schlick_pairs(T):
    """per (ir, face, which) of SCHLICK_ITEMS: two items whose cosines are neighbours in T, the first reflects by Schlick, the second
    refracts (the states of schlick_pairs)"""
    T = _t(T)
    key = ("shade_schlick", np.dtype(T).name)
    if key not in _cache:
        out = []
        for (ir, front, which), (hi, _, _) in zip(SCHLICK_ITEMS, schlick_pairs(T)):
            flat = one_sphere(DIELECTRIC, WHITE, ir, T)
            mk = lambda c: _shade(hi.what, flat, falling(c, T), UP, front, hi.state, T)
            a, b = bisect_flip(lambda c: mk(c).branch == "schlick", schlick_start(ratio_of(ir, front, T), T), T(1), T)
            out.append((mk(a), mk(b)))
        _cache[key] = out
    return _cache[key]


def shade_clamp_items(T):
    """head-on and perpendicular-ish hits of every (ir, face): d = -n towards the pole, and a ray that grazes it (s = 1 - 2^-12)"""
    T = _t(T)
    key = ("shade_clamp", np.dtype(T).name)
    if key not in _cache:
        state = state_with_uniform(0.5, T)
        out = []
        for ir, front in SCHLICK_CASES:
            flat = one_sphere(DIELECTRIC, WHITE, ir, T)
            face = "front" if front else "back"
            out.append(_shade(f"head-on ir={ir:.4g} {face}", flat, (0.0, -1.0, 0.0), UP, front, state, T))
            out.append(_shade(f"grazing ir={ir:.4g} {face}", flat, grazing(1 - 2.0 ** -12, T), UP, front, state, T))
        _cache[key] = out
    return _cache[key]


def shade_near_zero_pairs(T):
    """Lambertian hits whose normal is the unit vector at angle theta from -u (|n + u|^2 = 2 - 2 cos theta): theta = 0 (degenerate) and,
    per state, the two neighbouring theta in T between which the oracle's scatter changes from `degenerate` to `ball`"""
    T = _t(T)
    key = ("shade_near_zero", np.dtype(T).name)
    if key not in _cache:
        flat = one_sphere(LAMBERTIAN, (0.5, 0.25, 0.75), 0.0, T)
        exact, pairs = [], []
        for seed in (21, 22, 23):
            state = O.rng_stream(seed, 5, 0)
            u = ball_sample(state, T)[0].astype(np.float64)
            w = np.cross(u, [0.3, -0.5, 0.8])
            w /= np.linalg.norm(w)

            def mk(theta, u=u, w=w, state=state):
                n = -u * np.cos(float(theta)) + w * np.sin(float(theta))
                return _shade("near_zero behind a hit", flat, -n, n, True, state, T)
            exact.append(mk(T(0)))
            a, b = bisect_flip(lambda th: mk(th).branch == "degenerate", T(2.0 ** -12), T(2.0 ** -6), T)
            pairs.append((mk(a), mk(b)))
        _cache[key] = (exact, pairs)
    return _cache[key]


def shade_metal_items(T):
    """Metal hits of fuzz 0, 1 and 5"""
    T = _t(T)
    key = ("shade_metal", np.dtype(T).name)
    if key not in _cache:
        out = []
        for fz in (0.0, 1.0, 5.0):
            flat = one_sphere(METAL, (0.9, 0.8, 0.7), fz, T)
            for k, s in enumerate((0.1, 0.6, 0.95)):
                out.append(_shade(f"metal fuzz={fz:g}", flat, grazing(s, T), UP, True, O.rng_stream(43, k, int(fz)), T))
        _cache[key] = out
    return _cache[key]


def all_shades(T):
    exact, pairs = shade_near_zero_pairs(T)
    return ([s for p in shade_tir_pairs(T) for s in p] + [s for p in shade_schlick_pairs(T) for s in p] + list(shade_clamp_items(T))
            + list(exact) + [s for p in pairs for s in p] + list(shade_metal_items(T)))
