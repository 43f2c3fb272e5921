"""Scenes, rays and wave placements of the block-vote tests (tests/test_exact_vote.py on the CPU, tests/test_gpu_cull_vote.py on the GPU).
The model they are judged by is tests/exact_vote.py.  A helper module, not a conftest.py.

Everything here is a function of (scene, layout): the layout is unit op 28's answer, recorded in tests/golden/cull_layouts.npz for the CPU test
(which checks that the rays make the assertions bite) and read back from the device by the GPU test (which first checks it IS the recorded one)."""
import os
from fractions import Fraction

import numpy as np

import exact_vote as V

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cull_layouts.npz")
SCENES = ["flat_layer", "on_bin_edges", "two_clumps", "concentric", "big_class_8_plus_ground", "big_class_9_plus_ground", "far_from_origin", "one_block"]
FAMILIES = ["axis", "surface", "layer", "unreachable", "graze", "limits"]
LANES = (0, 5, 15, 16, 31, 32, 47, 48, 63)
MAX_POSITIONS = 1024            # items of an op-28 call: more than any layout of RTW_SINK_SPHERES spheres has positions


def tname(T):
    return "f32" if T is np.float32 else "f64"


def _cut(flat, keep):
    return {k: (int(keep.sum()) if k == "n" else np.asarray(v)[keep]) for k, v in flat.items()}


def scenes(T):
    """name -> flat scene of at most 512 spheres (the candidate sinks' limit): the vote scenes of test_gpu_round5, cut where needed, a class
    far from the origin, and a class of one block.  Float64: the coordinates are not binary32 values."""
    from test_gpu_round5 import _flat_scene, _vote_scenes
    src = _vote_scenes(T)
    out = {k: src[k] for k in SCENES if k in src}
    f = out["on_bin_edges"]                                      # 16 x 32 of the lattice: the boxes still end on bin edges (0.125 / 0.25 per bin)
    out["on_bin_edges"] = _cut(f, (f["cx"] >= -4) & (f["cx"] < 4) & (f["cz"] >= -18) & (f["cz"] < -2))
    rng = np.random.default_rng(31)
    n, off = 300, np.array([2000.0, -1000.0, 3000.0])
    out["far_from_origin"] = _flat_scene(T, off[0] + rng.uniform(-6, 6, n), off[1] + rng.uniform(-0.3, 0.3, n), off[2] + rng.uniform(-6, 6, n),
                                         rng.uniform(0.1, 0.3, n), 6)
    n = 20
    out["one_block"] = _flat_scene(T, rng.uniform(-2, 2, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-9, -5, n), rng.uniform(0.1, 0.3, n), 7)
    if T is np.float64:
        for name, f in out.items():
            if name != "on_bin_edges":                           # (the lattice keeps its exact edges)
                for key in ("cx", "cy", "cz", "r"):
                    f[key] = f[key] * (1 + 2.0 ** -40)
    assert all(f["n"] <= 512 for f in out.values())
    return {k: out[k] for k in SCENES}


def recorded_layout(name, T):
    z = np.load(GOLDEN)
    key = f"{name}_{tname(T)}"
    return V.Layout(z[key + "_idx"].astype(np.int64), z[key + "_inlane"].astype(bool), int(z[key + "_blocks"]))


# ---- the rays ---------------------------------------------------------------------------------------------------------------------
SMALL = [0.0, -0.0, 1e-10, -1e-10, 0.9e-9, -0.9e-9, 1.1e-9, -1.1e-9, 1e-6, -1e-6]      # direction components around the 1e-9 clamp of safe_inv
GRAZE_D = [(77 / 128, 102 / 128, 0.0), (0.5, 0.5, 181 / 256)]                          # short mantissas, |d|^2 = 0.9969 / 0.9999: o = q - 4 d is exact


GRAZES = {}                     # (scene, T) -> what rays() built its graze family from, in the family's order


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def rays(name, flat, model, T):
    """-> (family index [m], o [m, 3], d [m, 3]) as values of type T widened; built from the scene and the model's boxes with a fixed seed.
    The last two rays are the non-finite ones (a NaN direction, an infinite origin)."""
    import exact_filters as X
    rng = np.random.default_rng(1000 + SCENES.index(name))
    c, r = model.c, np.abs(model.r)
    glo, ghi = np.array([float(v) for v in model.glo]), np.array([float(v) for v in model.ghi])
    ext = ghi - glo
    size = float(ext.max())
    blo = {b: np.array([float(v) for v in model.lo[b]]) for b in model.finite}
    bhi = {b: np.array([float(v) for v in model.hi[b]]) for b in model.finite}
    fin = model.finite
    out = {f: [] for f in FAMILIES}

    def add(fam, o, d):
        out[fam].append((np.asarray(o, np.float64), np.asarray(d, np.float64)))

    def inside(lo, hi):
        return lo + rng.uniform(0.05, 0.95, 3) * (hi - lo)

    # axis: (nearly) axis-aligned directions -- one or two components from SMALL -- through the class, from inside it, from outside it on
    # either side, from exactly on its faces and on block faces; both signs of travel
    for a in range(3):
        b1, b2 = (a + 1) % 3, (a + 2) % 3
        for sg in (1.0, -1.0):
            starts = []
            for _ in range(3):
                starts.append(inside(glo, ghi))
            p = inside(glo, ghi); p[a] = glo[a] - 0.3 * size; starts.append(p)
            p = inside(glo, ghi); p[a] = ghi[a] + 0.3 * size; starts.append(p)
            p = inside(glo, ghi); p[a] = float(T(glo[a])); starts.append(p)
            p = inside(glo, ghi); p[a] = float(T(ghi[a])); starts.append(p)
            p = inside(glo, ghi); p[b1] = float(T(glo[b1])); starts.append(p)             # running IN a face of the class box
            p = inside(glo, ghi); p[b2] = float(T(ghi[b2])); starts.append(p)
            for b in [fin[i] for i in rng.choice(len(fin), min(3, len(fin)), replace=False)]:
                p = inside(blo[b], bhi[b]); p[a] = float(T(blo[b][a] if sg > 0 else bhi[b][a])); starts.append(p)   # on a block face, entering
                p = inside(blo[b], bhi[b]); p[b1] = float(T(bhi[b][b1])); starts.append(p)                          # sliding along a block face
            for j, p in enumerate(starts):
                d = np.zeros(3)
                d[b1] = SMALL[int(rng.integers(len(SMALL)))]
                if j % 2 == 0:
                    d[b2] = SMALL[int(rng.integers(len(SMALL)))]
                    d[a] = sg
                else:                                                                     # one small component, the other two generic
                    u = _unit(rng.normal(size=2))
                    d[a], d[b2] = sg * abs(u[0]), u[1]
                add("axis", p, d)
    # surface: origins on sphere surfaces (the ray after a bounce) going outwards, inwards, tangentially; origins inside block boxes
    for i in rng.choice(len(model.small), min(16, len(model.small)), replace=False):
        i = model.small[int(i)]
        nrm = _unit(rng.normal(size=3))
        p = c[i] + r[i] * nrm
        tan = _unit(np.cross(nrm, rng.normal(size=3)))
        for d in (nrm, -nrm, tan, _unit(nrm + rng.normal(size=3))):
            add("surface", p, d)
    for b in fin:
        add("surface", inside(blo[b], bhi[b]), _unit(rng.normal(size=3)))
    # layer: along the two longest axes of the class (inside it: the loose-bounds case) and across it
    order = np.argsort(ext)
    thin, w1, w2 = int(order[0]), int(order[1]), int(order[2])
    for _ in range(24):
        d = np.zeros(3)
        u = _unit(rng.normal(size=2))
        d[w1], d[w2], d[thin] = u[0], u[1], rng.choice([0.0, 1e-3, -1e-3, 0.02])
        add("layer", inside(glo, ghi), _unit(d) if d[thin] else d)
    for _ in range(24):
        p = inside(glo, ghi)
        sg = rng.choice([1.0, -1.0])
        p[thin] = (ghi[thin] + 0.5 * size) if sg < 0 else (glo[thin] - 0.5 * size)
        d = np.zeros(3)
        d[thin] = sg
        d[w1], d[w2] = rng.normal(size=2) * rng.choice([0.0, 0.05, 0.3])
        add("layer", p, _unit(d))
    # unreachable: beyond the class box and pointing away; rays whose LINE crosses a block box, but only at t < 0
    for a in range(3):
        for sg in (1.0, -1.0):
            for _ in range(4):
                p = inside(glo, ghi)
                p[a] = (ghi[a] if sg > 0 else glo[a]) + sg * rng.choice([0.02, 0.2, 2.0]) * size
                d = rng.normal(size=3) * 0.5
                d[a] = sg * (0.6 + abs(d[a]))
                add("unreachable", p, _unit(d))
    for b in fin:
        for j in range(3):
            q, d = inside(blo[b], bhi[b]), _unit(rng.normal(size=3))
            if j == 0 and len(fin) > 1:                                     # ... with another block ahead
                b2 = fin[(fin.index(b) + 1 + int(rng.integers(len(fin) - 1))) % len(fin)]
                d = _unit(inside(blo[b2], bhi[b2]) - q)
            with np.errstate(divide="ignore"):
                t_exit = float(np.min(np.where(d > 0, (bhi[b] - q) / d, np.where(d < 0, (blo[b] - q) / d, np.inf))))
            add("unreachable", q + (t_exit + rng.choice([1e-3, 0.02, 0.1]) * size) * d, d)
    # graze: rays through a corner / along past an edge of a block box -- the line meets the box in that point only -- then moved off it
    # outwards (and inwards) by an ulp, by hairs and by clear distances.  Constructed in rationals from the exact box, rounded to T once.
    pick = [fin[i] for i in rng.choice(len(fin), min(8, len(fin)), replace=False)]
    graze = GRAZES[(name, T)] = []                           # per graze ray: (the block it was built on, the shift)
    for b in pick:
        for which, gd in enumerate(GRAZE_D):
            sig = rng.choice([1, -1], 3)
            perm = rng.permutation(3)
            q = [(model.hi[b][k] if sig[k] > 0 else model.lo[b][k]) for k in range(3)]      # the corner with outward signs sig (Fractions)
            if which == 0:                                                                  # an edge: its middle on the third axis
                k3 = int(perm[2])
                q[k3] = (model.lo[b][k3] + model.hi[b][k3]) / 2
            d = np.zeros(3)
            d[perm[0]] = sig[perm[0]] * gd[0]                # leaves the box on this axis for t > 0 ...
            d[perm[1]] = -sig[perm[1]] * gd[1]               # ... and is outside it on these for t < 0
            d[perm[2]] = -sig[perm[2]] * gd[2]
            k0 = int(perm[0])
            for shift in (0.0, 1.0, -1.0, 1e-5, 1e-3, 0.02, 0.1, 0.4):      # ulps (+-1) or fractions of the class's size, outwards on axis k0
                o = [q[k] - 4 * Fraction(float(d[k])) for k in range(3)]
                if abs(shift) == 1.0:
                    # (an ulp of binary32 at the larger of |q| and |o|, for both precisions: the kernel sees the ray rounded to binary32)
                    o[k0] += int(shift * sig[k0]) * Fraction(2.0 ** (np.frexp(max(abs(float(q[k0])), abs(float(o[k0])), 1e-30))[1] - 24))
                elif shift:
                    o[k0] += Fraction(float(shift * sig[k0] * size))
                oT = [float(X.round_f32(v)) if T is np.float32 else float(v) for v in o]
                add("graze", oT, d)
                graze.append((b, shift))
    # limits: |d|^2 around the filter's 1.0009 and |o|_inf around its mf_o_max (1, 16, 31.9, 32.1 x the extent 2^8 / mf_sc), aimed at spheres
    s = X.mfma_scale(model.c, model.r)
    omax = X.mfma_ray_constants(s)[2]
    def aim(j, p):                                                          # at a sphere's rim, or (every third ray) past the whole class
        i = model.small[int(rng.integers(len(model.small)))]
        return _unit(c[i] + (r[i] if j % 3 else 2.0 * size) * _unit(rng.normal(size=3)) - p)

    for s2 in (1 - 2.0 ** -20, 1 + 3e-7, 1.00089, 1.0201):
        for j in range(6):
            p = inside(glo - 0.3 * size, ghi + 0.3 * size)
            add("limits", p, aim(j, p) * np.sqrt(s2))
    for mult in (1.0, 16.0, 31.9, 32.1):
        for j in range(6):
            u = rng.normal(size=3)
            p = u / np.abs(u).max() * omax * mult / 32.0
            add("limits", p, aim(j, p))
    add("limits", inside(glo, ghi), [0.0, np.nan, 1.0])
    add("limits", [np.inf, 0.0, 0.0], [0.0, 0.0, -1.0])
    fam = np.concatenate([[FAMILIES.index(f)] * len(out[f]) for f in FAMILIES])
    with np.errstate(over="ignore"):
        o = np.array([p for f in FAMILIES for p, _ in out[f]]).astype(T).astype(np.float64)
        d = np.array([q for f in FAMILIES for _, q in out[f]]).astype(T).astype(np.float64)
    return fam, o, d


def far_miss(model, T):
    """a unit ray above the class box that points away from it: on its own it votes for the infinite boxes only"""
    glo, ghi = np.array([float(v) for v in model.glo]), np.array([float(v) for v in model.ghi])
    o = (glo + ghi) / 2
    o[1] = ghi[1] + model.rs + 1.0
    return o.astype(T).astype(np.float64), np.array([0.0, 1.0, 0.0])


def as_kernel(v):
    """a ray's components as block_sets sees them: rounded to binary32, for both precisions"""
    with np.errstate(over="ignore"):
        return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


_JUDGED = {}


def judged(name, T, layout=None):
    """(flat, model, fam, o, d, ok, must, may, far_o, far_d) of a scene, computed once: must / may are lists of frozensets (None for the non-finite
    rays), from the recorded layout unless one is given"""
    key = (name, T)
    if key not in _JUDGED:
        import exact_filters as X
        flat = scenes(T)[name]
        model = V.Model(flat, layout or recorded_layout(name, T), T)
        fam, o, d = rays(name, flat, model, T)
        ok = X.f32_mf_ok(o, d, X.mfma_scale(model.c, model.r))
        finite = np.isfinite(o).all(1) & np.isfinite(d).all(1)
        must, may = [], []
        for j in range(len(o)):
            if not finite[j]:
                must.append(None); may.append(None)
                continue
            a, b = model.expected(as_kernel(o[j]), as_kernel(d[j]), bool(ok[j]))
            must.append(a); may.append(b)
        fo, fd = far_miss(model, T)
        _JUDGED[key] = (flat, model, fam, o, d, ok, must, may, fo, fd)
    return _JUDGED[key]


# ---- the waves ---------------------------------------------------------------------------------------------------------------------
def placements():
    """name -> the lanes of a wave that hold the ray under test (every other lane holds the far-miss ray)"""
    out = {f"lane{l}": [l] for l in LANES}
    out.update({f"row{q}": list(range(16 * q, 16 * q + 16)) for q in range(4)})
    out.update({f"half{h}": list(range(32 * h, 32 * h + 32)) for h in range(2)})
    return out


def waves(o, d, far_o, far_d, lanes, tmin):
    """one wave per ray: the ray in `lanes`, the far-miss ray elsewhere -> the [m * 64, 8] input slots of ops 14 / 27"""
    m = len(o)
    x = np.empty((m, 64, 8))
    x[:, :, 0:3], x[:, :, 3:6] = far_o, far_d
    x[:, lanes, 0:3], x[:, lanes, 3:6] = o[:, None, :], d[:, None, :]
    x[:, :, 6], x[:, :, 7] = tmin, np.inf
    return x.reshape(m * 64, 8)
