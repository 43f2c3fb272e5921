"""Scenes too large for the LDS scene copy, their cameras, and the table of kernel instances they reach (a plain helper module).

The trace kernel stages the scene in LDS only while scene_geom_alloc(n, n_pad) entries fit RTW_LDS_SCENE_MAX_BYTES = 24 KB
(csrc/rtw_scan.hpp, csrc/rtw_launch.hip): 1536 entries of 16 B in Float32, 768 of 32 B in Float64, of which 8 are the prefetch tail and
n_pad is n rounded up to the scan group -- so the plain scans stage at most 1528 / 760 spheres.  Larger scenes run the LDS_SCENE = false
instances, which gather pass 2 from global memory.  `CASES` lists, per (entry point, precision, size, scan flags), the instance the
launch must report on its `[rtw debug] trace instance:` / `features instance:` line (RTW_ENABLE_TEST_AIDS=1 RTW_DEBUG=1);
tests/test_gpu_global_scene.py compares every row with the CPU oracle and probes, in a fresh process, that the row reached that instance.

Group cull leaves LDS earlier (its layout holds the exact-test copies, their indices and, on the matrix pipe, the block vote's tables);
where it does depends on the scene.  GROUP_CULL_FIRST_GLOBAL_N records it for big_scene(n, T, 7); nothing asserts it."""
from collections import namedtuple

import numpy as np

F32_BIG, F64_BIG = 1600, 800
BIG = {np.float32: F32_BIG, np.float64: F64_BIG}
#: (the largest scene of the plain scans that is staged in LDS, the smallest that is not)
BOUNDARY = {np.float32: (1528, 1529), np.float64: (760, 761)}
PRECISIONS = [np.float32, np.float64]
#: rtw_params.flags: matrix pipe, all-VALU (RTW_FLAG_SCAN_VALU), group cull on the matrix pipe (RTW_FLAG_GROUP_CULL), group cull all-VALU
FLAGS = (0, 4, 1, 5)
FEATURE_FLAGS = (0, 4, 1)
SCENE_SEED = 7
#: (precision, flags) -> the first n at which a render of big_scene(n, T, SCENE_SEED) under group cull reported lds_scene=0, found by
#: bisection over the debug line on an MI355X (lds_scene=1 for the 6 sizes below it, 0 for the 6 above; lds_bytes 43744 -> 19264 at Float32
#: flags 1).  A record, not asserted: at the boundary sizes of the plain scans group cull is in global memory on both sides.
GROUP_CULL_FIRST_GLOBAL_N = {("f32", 1): 1154, ("f32", 5): 1282, ("f64", 1): 642, ("f64", 5): 642}

# caller indices of the spheres the tests look at
HOLLOW_OUTER, HOLLOW_INNER, MIRROR = 1, 2, 3


def pair_indices(n):
    """the coincident pair: two spheres of one centre and radius and two albedos, far apart in the caller's list"""
    return 5, n - 3


#: where the special spheres stand (x, z; they rest on the ground): in front of all three cameras
_PAIR_XZ, _HOLLOW_XZ, _MIRROR_XZ = (0.9, -0.7), (-0.2, -1.5), (0.3, -2.4)
_SPECIAL_R = 0.25


def big_scene(n, T, seed=SCENE_SEED):
    """-> flat scene dict of n >= 16 spheres: index 0 the ground (radius 1000), the others of radius 0.05 .. 0.25 resting on it over
    x, z in -8 .. 8, Lambertian / Metal (fuzz in [0, 0.5]) / Dielectric mixed; index 1 / 2 a hollow glass sphere (radius 0.25 with
    radius -0.2 inside); index 3 a Metal sphere of fuzz exactly 0; indices 5 and n - 3 one sphere of two albedos (pair_indices)"""
    assert n >= 16
    T = np.dtype(T).type
    rng = np.random.default_rng(seed)
    specials = np.array([_PAIR_XZ, _HOLLOW_XZ, _MIRROR_XZ])
    x, z = np.empty(n), np.empty(n)
    for k in range(n):                       # keep the random spheres off the special ones, so those stay in the picture
        while True:
            x[k], z[k] = rng.uniform(-8, 8, 2)
            if np.min(np.hypot(specials[:, 0] - x[k], specials[:, 1] - z[k])) > 0.55:
                break
    r = rng.uniform(0.05, 0.25, n)
    kind = rng.integers(0, 3, n).astype(np.int32)
    alb = rng.uniform(0.1, 0.9, (n, 3))
    param = np.where(kind == 1, rng.uniform(0, 0.5, n), np.where(kind == 2, 1.5, 0.0))
    y = r.copy()

    def put(i, xz, radius, k, albedo, p):
        x[i], z[i], y[i], r[i], kind[i], param[i] = xz[0], xz[1], _SPECIAL_R, radius, k, p
        alb[i] = albedo

    x[0], y[0], z[0], r[0], kind[0], param[0] = 0.0, -1000.0, 0.0, 1000.0, 0, 0.0
    alb[0] = (0.5, 0.5, 0.5)
    put(HOLLOW_OUTER, _HOLLOW_XZ, _SPECIAL_R, 2, (1.0, 1.0, 1.0), 1.5)
    put(HOLLOW_INNER, _HOLLOW_XZ, -0.2, 2, (1.0, 1.0, 1.0), 1.5)
    put(MIRROR, _MIRROR_XZ, _SPECIAL_R, 1, (0.8, 0.8, 0.9), 0.0)
    first, second = pair_indices(n)
    put(first, _PAIR_XZ, _SPECIAL_R, 0, (0.9, 0.1, 0.1), 0.0)
    put(second, _PAIR_XZ, _SPECIAL_R, 0, (0.1, 0.1, 0.9), 0.0)
    return dict(n=n, cx=x.astype(T), cy=y.astype(T), cz=z.astype(T), r=r.astype(T), kind=kind, ar=alb[:, 0].astype(T), ag=alb[:, 1].astype(T),
                ab=alb[:, 2].astype(T), param=param.astype(T))


def swapped_pair(flat):
    """the scene with the two albedos of the coincident pair exchanged"""
    first, second = pair_indices(flat["n"])
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in flat.items()}
    for k in ("ar", "ag", "ab"):
        out[k][first], out[k][second] = flat[k][second], flat[k][first]
    return out


def solid_glass(flat):
    """the scene without the hollow: the inner sphere of the glass sphere shrunk to nothing visible (radius -1e-3)"""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in flat.items()}
    out["r"][HOLLOW_INNER] = -1e-3
    return out


_scenes = {}


def scene(T, n=None, seed=SCENE_SEED):
    """big_scene, computed once per (n, T, seed); read-only"""
    T = np.dtype(T).type
    n = BIG[T] if n is None else n
    key = (n, np.dtype(T).name, seed)
    if key not in _scenes:
        flat = big_scene(n, T, seed)
        for v in flat.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _scenes[key] = flat
    return _scenes[key]


VIEW_SEEDS = (3, 14, 1234570)


def cameras(T):
    """the camera set: cfg2's golden camera cast to T, t_cam2, t_default_cam"""
    import rtw_amd
    from conftest import CamObj, load_golden
    T = np.dtype(T).type
    g = load_golden("cfg2_random_320x180_64spp_d16_f32", numerics="reference")
    cam = {k: (np.asarray(v).astype(T) if np.ndim(v) else T(v)) for k, v in g["cam"].items()}
    return [CamObj(cam), rtw_amd.t_cam2(elem_type=T), rtw_amd.t_default_cam(elem_type=T)]


def camera_dict(cam):
    """a camera of the set as the dict tests/features_ref.py and the oracle's unit calls take"""
    return {k: getattr(cam, k) for k in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w", "lens_radius")}


# ---- the instance table ----------------------------------------------------------------------------------------------------------------
#: what a `[rtw debug] ... instance:` line says, without its lds_bytes / blocks_per_cu; lds_scene None: not asserted (group cull at the
#: boundary sizes of the plain scans)
Instance = namedtuple("Instance", "kernel prec lds_scene cull mfma fixed batch accum adapt")
Case = namedtuple("Case", "entry T n flags expect")

#: entry point -> (batch, accum, adapt) of the trace instance it launches
TRACE_ENTRIES = {"render": (0, 0, 0), "batch": (1, 0, 0), "accum": (0, 1, 0), "adapt": (0, 1, 1), "batch_accum": (1, 1, 0), "batch_adapt": (1, 1, 1)}
FEATURE_ENTRIES = ("features_host", "features_device")


def _prec(T):
    return "f64" if np.dtype(T) == np.float64 else "f32"


def _trace_case(entry, T, n, flags, lds):
    cull, mfma = flags & 1, 0 if flags & 4 else 1
    b, a, d = TRACE_ENTRIES[entry]
    fixed = (lds if mfma else 0)                          # (the probe runs in the default numerics mode; None: follows lds_scene, not asserted)
    return Case(entry, T, n, flags, Instance("trace", _prec(T), lds, cull, mfma, fixed, b, a, d))


def _cases():
    rows = []
    for T in PRECISIONS:
        for entry in ("batch", "accum", "adapt", "batch_accum", "batch_adapt"):
            for flags in FLAGS:
                rows.append(_trace_case(entry, T, BIG[T], flags, 0))
        for entry in FEATURE_ENTRIES:
            for flags in FEATURE_FLAGS:              # (the feature kernel has no cull layout: flags 1 runs flags 0's instance)
                rows.append(Case(entry, T, BIG[T], flags, Instance("features", _prec(T), 0, 0, 0 if flags & 4 else 1, 0, 0, 0, 0)))
        for k, n in enumerate(BOUNDARY[T]):
            for entry in ("render", "accum"):
                for flags in FLAGS:
                    rows.append(_trace_case(entry, T, n, flags, None if flags & 1 else 1 - k))
    return rows


CASES = _cases()


def cases(entry, big_only=True):
    """the rows of one entry point (pytest.param with readable ids)"""
    import pytest
    out = []
    for c in CASES:
        if c.entry == entry and (not big_only or c.n == BIG[c.T]):
            out.append(pytest.param(c, id=f"{entry.split('_')[-1] + '-' if entry in FEATURE_ENTRIES else ''}{_prec(c.T)}-n{c.n}-flags{c.flags}"))
    return out


def boundary_cases():
    import pytest
    return [pytest.param(c, id=f"{c.entry}-{_prec(c.T)}-n{c.n}-flags{c.flags}") for c in CASES if c.n != BIG[c.T]]


def global_instances():
    """every shipped instance this module is about: the 40 trace tuples with lds_scene=0 and batch | accum, the 4 feature tuples"""
    want = set()
    for prec in ("f32", "f64"):
        for cull in (0, 1):
            for mfma in (0, 1):
                for b, a, d in ((1, 0, 0), (0, 1, 0), (0, 1, 1), (1, 1, 0), (1, 1, 1)):
                    want.add(Instance("trace", prec, 0, cull, mfma, 0, b, a, d))
        for mfma in (0, 1):
            want.add(Instance("features", prec, 0, 0, mfma, 0, 0, 0, 0))
    return want


def parse_instance_lines(stderr_text):
    """the `[rtw debug] trace instance:` / `features instance:` lines of a process's stderr -> [(Instance, lds_bytes, blocks_per_cu)]"""
    import re
    out = []
    pat = re.compile(r"\[rtw debug\] (trace|features) instance: (f32|f64) lds_scene=(\d) cull=(\d) mfma=(\d) fixed=(\d) batch=(\d) accum=(\d) adapt=(\d) "
                     r"lds_bytes=(\d+) blocks_per_cu=(\d+)\s*$")
    for ln in stderr_text.splitlines():
        m = pat.search(ln)
        if m:
            out.append((Instance(m.group(1), m.group(2), *[int(m.group(k)) for k in range(3, 10)]), int(m.group(10)), int(m.group(11))))
    return out


def matches(got, expect):
    """an Instance a launch reported against a row's (None fields are not asserted)"""
    return all(e is None or g == e for g, e in zip(got, expect))


def launch(case, width=8, height=5, spp=2, depth=8):
    """One call of the row's entry point on the row's scene (a tiny frame: the probe only needs the launch to happen).  The batched
    entries take the first two cameras."""
    import test_gpu_accum_batch as AB
    import test_gpu_batch as B
    import test_gpu_features as F
    from test_gpu_adaptive import UNREACHABLE, Ad, single
    T, flat = case.T, scene(case.T, case.n)
    cams = cameras(T)
    if case.entry == "render":
        single(flat, cams[0], T, width, height, spp, depth, 3, n_chunks=spp, flags=case.flags)
    elif case.entry == "batch":
        B.batch(flat, cams[:2], list(VIEW_SEEDS[:2]), T, width, height, spp, depth, n_chunks=spp, flags=case.flags)
    elif case.entry in ("accum", "adapt"):
        a = Ad(flat, cams[0], T, width, height, spp, depth, 3, n_chunks=spp, min_chunks=2, check_chunks=2)
        try:
            if case.entry == "accum":
                P, Cm = a._params(case.flags), a.C.make_camera(a.cam, T)
                import ctypes as C
                fn = a.L.rtw_render_accum_f64 if T is np.float64 else a.L.rtw_render_accum_f32
                a.C.check(fn(a.scene, C.byref(Cm), C.byref(P), 0, spp, a.acc, None, None))
            else:
                a.run_ok(UNREACHABLE, flags=case.flags)
        finally:
            a.close()
    elif case.entry in ("batch_accum", "batch_adapt"):
        vs = [Ad(flat, cams[v], T, width, height, spp, depth, VIEW_SEEDS[v], n_chunks=spp, min_chunks=2, check_chunks=2) for v in range(2)]
        try:
            if case.entry == "batch_accum":
                AB.ok(AB.batch_accum(vs, 0, spp, flags=case.flags), vs[0])
            else:
                AB.ok(AB.batch_adapt(vs, UNREACHABLE, flags=case.flags), vs[0])
        finally:
            AB.close(vs)
    elif case.entry == "features_host":
        F.features_host(flat, camera_dict(cams[0]), T, width, height, spp, spp, (0, spp), seed=3, flags=case.flags)
    elif case.entry == "features_device":
        with F.DeviceScene(flat, T) as ds:
            ds.features(camera_dict(cams[0]), width, height, spp, spp, (0, spp), seed=3, flags=case.flags)
    else:
        raise ValueError(case.entry)


# ---- the adaptive case: 48 x 27 (24 tiles, a ragged last row), 32 chunks of one sample, checkpoints 8 / 16 / 24 -------------------------
AD_W, AD_H, AD_SPP, AD_DEPTH, AD_SEED, AD_FLOOR = 48, 27, 32, 8, 7, 0.03
AD_CHECKS = [8, 16, 24]
_adaptive = {}


def adaptive_case(oracle, T):
    """The oracle's samples of every pixel of the adaptive frame (cfg2's camera), the words they give at every checkpoint, the tiles'
    ratios D / M there and a tolerance picked from those ratios as tests/test_gpu_adaptive.py case48 picks it: the middle of the gap
    between neighbouring ratios (at least 1e-6 relative from every ratio) that maximises the smallest of the three groups -- tiles
    that stop at the first checkpoint, at a later one, never.  Computed once per precision; read-only."""
    from rtw_amd import reference_decisions
    from test_gpu_adaptive import all_samples, oracle_words
    T = np.dtype(T).type
    if T in _adaptive:
        return _adaptive[T]
    flat, cam = scene(T), cameras(T)[0]
    samples = all_samples(oracle, flat, cam, T, AD_W, AD_H, AD_SPP, AD_DEPTH, AD_SEED, AD_SPP)
    words_at = oracle_words(samples, 1, AD_CHECKS + [AD_SPP])
    ratios = {}
    for c in AD_CHECKS:
        _, D, Y, M = reference_decisions(words_at[c], AD_W, AD_H, c, 1.0, AD_FLOOR, return_terms=True)
        ratios[c] = np.array([d / m for d, m in zip(D, M)])
    allr = np.sort(np.unique(np.concatenate(list(ratios.values()))))
    tol, best = None, -1
    for lo, hi in zip(allr[:-1], allr[1:]):
        cand = 0.5 * (lo + hi)
        if min(abs(allr - cand) / cand) <= 1e-6:
            continue
        first, later, never = stop_groups(ratios, cand)
        score = min(first.sum(), later.sum(), never.sum())
        if score > best:
            tol, best = cand, score
    out = dict(flat=flat, cam=cam, T=T, samples=samples, words_at=words_at, ratios=ratios, tol=float(tol))
    _adaptive[T] = out
    return out


def stop_groups(ratios, tol):
    """-> bool arrays over the tiles: stops at the first checkpoint, at a later one, never"""
    first = ratios[AD_CHECKS[0]] <= tol
    never = np.all([ratios[c] > tol for c in AD_CHECKS], axis=0)
    return first, ~first & ~never, never
