"""The conditions that keep tests/test_gpu_material_sweep.py from being vacuous, on the CPU oracle alone: the sweep scene's paths really
refract, reflect by Schlick and reflect totally on many spheres and both faces, and every edge builder of tests/material_sweep.py
returns inputs that the oracle puts on BOTH sides of the decision it is named after."""
import numpy as np
import pytest

import material_sweep as MS

F = MS.PRECISIONS
IDS = ["f32", "f64"]


@pytest.mark.parametrize("extra", [0, 24])
@pytest.mark.parametrize("T", F, ids=IDS)
def test_census_floors(oracle, T, extra):
    """64 x 36, depth 16, the first sample of every pixel; the floors hold for the first 18 spheres with and without the 24 extra ones"""
    flat, _ = MS.sweep_scene(T, extra)
    assert flat["n"] == MS.N_BASE + extra
    c = MS.census_cached(T, extra)
    print({k: v[:MS.N_BASE].tolist() for k, v in c.items()})
    for i in MS.DIELECTRICS:
        assert c["refract"][i, 0] >= 10 and c["refract"][i, 1] >= 10, (i, c["refract"][i].tolist())
    sch, tir = c["schlick"][:MS.N_BASE].sum(axis=1), c["tir"][:MS.N_BASE].sum(axis=1)
    assert sch.sum() >= 50 and (sch > 0).sum() >= 5, sch.tolist()
    assert tir.sum() >= 50 and (tir > 0).sum() >= 3, tir.tolist()
    for i in [MS.GROUND] + MS.METALS + MS.LAMBERTIANS:
        assert c["ball"][i] >= 10, (i, c["ball"].tolist())
    for k in ("tir", "schlick", "refract"):
        assert not c[k][[MS.GROUND] + MS.METALS + MS.LAMBERTIANS].any()
    assert not c["ball"][MS.DIELECTRICS].any()


def test_the_extra_spheres_make_a_second_block(oracle):
    flat, _ = MS.sweep_scene(np.float32, 24)
    assert flat["n"] > 32 and MS.sweep_scene(np.float32)[0]["n"] < 32
    r = flat["r"][MS.N_BASE:].astype(np.float64)
    assert not np.any(np.log2(r) == np.round(np.log2(r)))
    assert MS.census_cached(np.float32, 24)["ball"][MS.N_BASE:].sum() > 0          # (in view)


def _next(x, T):
    return MS.from_ordinal(MS.to_ordinal(x, T) + 1, T)


@pytest.mark.parametrize("T", F, ids=IDS)
def test_tir_pairs_flip_between_neighbours(oracle, T):
    pairs = MS.tir_pairs(T)
    assert len(pairs) == len(MS.TIR_CASES)
    for (ir, front), (lo, hi) in zip(MS.TIR_CASES, pairs):
        assert hi.d[0] == _next(lo.d[0], T) and lo.front == hi.front == front
        assert MS.branch_of(lo, T) == "refract" and MS.branch_of(hi, T) == "tir", lo.what
        # one flip within +- 100 neighbours
        k0 = MS.to_ordinal(lo.d[0], T)
        flips = 0
        prev = None
        for k in range(k0 - 100, k0 + 102):
            b = MS.branch_of(lo._replace(d=MS.grazing(MS.from_ordinal(k, T), T)), T) == "tir"
            flips += prev is not None and b != prev
            prev = b
        assert flips == 1, (lo.what, flips)
    if T is np.float32:         # ir = 0.75 from outside: ratio * sin_t is exactly 1 at s = 0.75 -- `>` and `>=` part here
        lo, hi = pairs[1]
        assert lo.d[0] == np.float32(0.75)


@pytest.mark.parametrize("T", F, ids=IDS)
def test_schlick_pairs_flip_between_neighbours(oracle, T):
    pairs = MS.schlick_pairs(T)
    assert len(pairs) == len(MS.SCHLICK_ITEMS) == 2 * len(MS.SCHLICK_CASES)
    for (ir, front, which), (hi, lo, u) in zip(MS.SCHLICK_ITEMS, pairs):
        assert -lo.d[1] == _next(-hi.d[1], T)
        assert MS.branch_of(hi, T) == "schlick" and MS.branch_of(lo, T) == "refract", hi.what
        ratio = MS.ratio_of(ir, front, T)
        assert oracle.reflectance(-hi.d[1], ratio, T) > u and not oracle.reflectance(-lo.d[1], ratio, T) > u
        if which == "low":          # the first uniform above r0
            r0 = float(oracle.reflectance(T(1), ratio, T))
            assert r0 < float(u) <= r0 + (2.0 ** -52 if T is np.float64 else 2.0 ** -23)


@pytest.mark.parametrize("T", F, ids=IDS)
def test_clamp_inputs_are_on_and_past_the_clamp(oracle, T):
    T = np.dtype(T).type
    seen = set()
    for b in MS.clamp_inputs(T):
        cos = -((b.d[0] * b.n[0] + b.d[1] * b.n[1]) + b.d[2] * b.n[2])
        branch, out, _ = MS.classify(b.kind, b.albedo, b.param, b.d, MS.rec8(b.n, b.front, T), b.state, T)
        assert np.isfinite(out).all(), b.what
        if b.what.startswith("clamped"):
            assert cos > T(1)
            assert branch != "tir"
        elif b.what.startswith("head-on"):
            assert abs(float(cos) - 1) < 4 * np.finfo(T).eps and branch != "tir"
        else:
            assert cos == 0 and (branch == "tir") == (MS.ratio_of(b.param, b.front, T) > 1)
        seen.add(branch)
    assert seen == {"tir", "schlick", "refract"}


@pytest.mark.parametrize("T", F, ids=IDS)
def test_near_zero_inputs_lie_on_both_sides(oracle, T):
    exact, pairs = MS.near_zero_inputs(T)
    assert len(exact) == 3 and len(pairs) == 3
    for b in exact:
        u, _ = MS.ball_sample(b.state, T)
        assert np.array_equal(b.n + u, np.zeros(3, T))
        branch, out, _ = MS.classify(b.kind, b.albedo, b.param, b.d, MS.rec8(b.n, b.front, T), b.state, T)
        assert branch == "degenerate" and MS._same(out[3:6], b.n)
        n2 = float((b.n[0] * b.n[0] + b.n[1] * b.n[1]) + b.n[2] * b.n[2])
        assert abs(n2 - 1) < 8 * np.finfo(T).eps
    for axis, (lo, hi) in enumerate(pairs):
        assert hi.n[axis] == _next(lo.n[axis], T)
        assert MS.branch_of(lo, T) == "degenerate" and MS.branch_of(hi, T) == "ball"
        u, _ = MS.ball_sample(lo.state, T)
        for b, below in ((lo, True), (hi, False)):
            v = b.n + u
            assert oracle.near_zero(v, T) == below
            assert abs(float((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) - 1e-5) < 1e-7


@pytest.mark.parametrize("T", F, ids=IDS)
def test_metal_of_fuzz_zero_leaves_the_normalised_mirror_direction(oracle, T):
    seen = set()
    for b in MS.metal_inputs(T):
        branch, out, s1 = MS.classify(b.kind, b.albedo, b.param, b.d, MS.rec8(b.n, b.front, T), b.state, T)
        assert branch == "ball" and not np.array_equal(s1, b.state)           # (fuzz 0 draws its unit vector all the same)
        assert MS._same(out[6:9], np.asarray(b.albedo, dtype=T))
        mirror = MS.normalize_t(oracle.reflect(b.d, b.n, T), T)
        if float(b.param) == 0:
            assert MS._same(out[3:6], mirror), b.what
        else:
            assert not MS._same(out[3:6], mirror), b.what
        seen.add(float(b.param))
    assert seen == {0.0, 1.0, 5.0}


@pytest.mark.parametrize("T", F, ids=IDS)
def test_the_items_of_op_26_lie_on_both_sides_behind_a_real_hit(oracle, T):
    """the same decisions with hit_world and its hit record in front of scatter"""
    for (ir, front), (lo, hi) in zip(MS.TIR_CASES, MS.shade_tir_pairs(T)):
        assert hi.d[0] == _next(lo.d[0], T)
        assert lo.branch == "refract" and hi.branch == "tir", lo.what
    for lo, hi in MS.shade_schlick_pairs(T):
        assert -hi.d[1] == _next(-lo.d[1], T)
        assert lo.branch == "schlick" and hi.branch == "refract", lo.what
    assert {s.branch for s in MS.shade_clamp_items(T)} == {"tir", "schlick", "refract"}
    exact, pairs = MS.shade_near_zero_pairs(T)
    assert all(s.branch == "degenerate" for s in exact)
    for lo, hi in pairs:
        assert lo.branch == "degenerate" and hi.branch == "ball"
        assert not MS._same(lo.o, hi.o)
    assert all(s.branch == "ball" for s in MS.shade_metal_items(T))
    for s in MS.all_shades(T):
        again = MS.shade_branch(s.flat, s.o, s.d, s.state, T)
        assert again[0] == s.branch and again[1] == 0
