"""The shading half of the trace kernel across the material parameter space (tests/material_sweep.py), against the CPU oracle.

Unit level: ops 1 - 4 and op 26 -- one bounce as the trace kernel composes it, on the material rows the upload made -- on the inputs that
sit on either side of every decision of scatter (total internal reflection, Schlick's comparison, the cosine clamp, near_zero, fuzz 0).
The oracle's own answer says which branch an input takes, and each test asserts that both sides of its threshold were among the inputs
it sent.  Render level: the sweep scene (refraction indices 0.667 .. 4, bubbles, fuzz 0 .. 3, albedos 0 .. 1.5) through every entry point
and scan mode.  Every comparison is on the bits.  Tolerance: NONE."""
import numpy as np
import pytest

import features_ref as FR
import material_sweep as MS
import test_gpu_accum as PA
import test_gpu_batch as B
import test_gpu_features as GF
from conftest import CamObj
from test_gpu_adaptive import UNREACHABLE, Ad
from test_gpu_pool import FLAG_POOL, needs_pool
from test_gpu_units import run_unit

pytestmark = pytest.mark.gpu
F = MS.PRECISIONS
IDS = ["f32", "f64"]
SEED = 5
#: (width, height, spp, n_chunks, depth)
FRAME_A, FRAME_B = (64, 36, 8, 4, 16), (61, 37, 3, 0, 50)
FRAMES = {"64x36": FRAME_A, "61x37": FRAME_B}
_refs = {}


def _bits_equal(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    bad = FR.bits(got) != FR.bits(ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ from the oracle; first at {np.argwhere(bad)[:4].tolist()}"


def _wide(v):
    return np.asarray(v).astype(np.float64)


# ---- unit level ---------------------------------------------------------------------------------------------------------------------------
def _cos_of(b, T):
    """the clamped cosine scatter hands to reflectance, in T"""
    T = np.dtype(T).type
    c = -((b.d[0] * b.n[0] + b.d[1] * b.n[1]) + b.d[2] * b.n[2])
    return c if T(1) > c else T(1)


@pytest.mark.parametrize("T", F, ids=IDS)
def test_reflect_refract_reflectance_on_the_edge_inputs(oracle, T):
    bs = MS.all_bounces(T)
    diel = [b for b in bs if b.kind == MS.DIELECTRIC]
    y1 = run_unit(1, np.array([[*_wide(b.d), *_wide(b.n)] for b in bs]), 3, T)
    for b, y in zip(bs, y1):
        _bits_equal(y.astype(T), oracle.reflect(b.d, b.n, T), f"reflect, {b.what}")
    ratios = [MS.ratio_of(b.param, b.front, T) for b in diel]
    y2 = run_unit(2, np.array([[*_wide(b.d), *_wide(b.n), float(r)] for b, r in zip(diel, ratios)]), 3, T)
    y3 = run_unit(3, np.array([[float(_cos_of(b, T)), float(r)] for b, r in zip(diel, ratios)]), 1, T)
    for b, r, ya, yb in zip(diel, ratios, y2, y3):
        _bits_equal(ya.astype(T), oracle.refract(b.d, b.n, r, T), f"refract, {b.what}")
        _bits_equal(yb.astype(T), np.array([oracle.reflectance(_cos_of(b, T), r, T)]), f"reflectance, {b.what}")
    # Schlick's comparison on the device's own reflectance: above u for one neighbour, not for the other
    by_input = {id(b): float(y[0]) for b, y in zip(diel, y3)}
    for hi, lo, u in MS.schlick_pairs(T):
        assert by_input[id(hi)] > float(u) and not by_input[id(lo)] > float(u), hi.what


def _scatter_rows(bs, T):
    return np.array([[*b.state.view(np.float64), float(b.kind), *_wide(np.asarray(b.albedo, dtype=T)), float(b.param), *_wide(b.d),
                      *_wide(MS.rec8(b.n, b.front, T))] for b in bs])


@pytest.mark.parametrize("T", F, ids=IDS)
def test_scatter_on_both_sides_of_every_decision(oracle, T):
    bs = MS.all_bounces(T)
    y = run_unit(4, _scatter_rows(bs, T), 11, T)
    branch = {}
    for b, row in zip(bs, y):
        br, out, s1 = MS.classify(b.kind, b.albedo, b.param, b.d, MS.rec8(b.n, b.front, T), b.state, T)
        branch[id(b)] = br
        _bits_equal(row[2:11].astype(T), out, f"{b.what} ({br})")
        assert np.array_equal(row[:2].view(np.uint64), s1), (b.what, br)
    for lo, hi in MS.tir_pairs(T):
        assert (branch[id(lo)], branch[id(hi)]) == ("refract", "tir"), lo.what
    for hi, lo, _ in MS.schlick_pairs(T):
        assert (branch[id(hi)], branch[id(lo)]) == ("schlick", "refract"), hi.what
    exact, pairs = MS.near_zero_inputs(T)
    assert all(branch[id(b)] == "degenerate" for b in exact)
    for lo, hi in pairs:
        assert (branch[id(lo)], branch[id(hi)]) == ("degenerate", "ball")
    assert {branch[id(b)] for b in MS.clamp_inputs(T)} == {"tir", "schlick", "refract"}
    assert {float(b.param) for b in MS.metal_inputs(T)} == {0.0, 1.0, 5.0}


@pytest.mark.parametrize("T", F, ids=IDS)
def test_one_bounce_as_the_kernel_composes_it(oracle, T):
    """op 26: hit_world, then the trace kernel's own sequence with the constants the upload stored (1 / ir, r0 of both faces) -- against
    the oracle's hit_world + scatter, which derive them from ir at every hit.  One launch per one-sphere scene."""
    items = MS.all_shades(T)
    scenes = {}
    for s in items:
        scenes.setdefault(id(s.flat), []).append(s)
    sent = {}
    for group in scenes.values():
        x = np.array([[*s.state.view(np.float64), *_wide(s.o), *_wide(s.d)] for s in group])
        y = run_unit(26, x, 12, T, flat=group[0].flat)
        for s, row in zip(group, y):
            br, idx, out, s1, _ = MS.shade_branch(s.flat, s.o, s.d, s.state, T)
            sent[id(s)] = br
            assert int(row[2]) == idx == 0, s.what
            _bits_equal(row[3:12].astype(T), out, f"{s.what} ({br})")
            assert np.array_equal(row[:2].view(np.uint64), s1), (s.what, br)
    for lo, hi in MS.shade_tir_pairs(T):
        assert (sent[id(lo)], sent[id(hi)]) == ("refract", "tir"), lo.what
    for lo, hi in MS.shade_schlick_pairs(T):
        assert (sent[id(lo)], sent[id(hi)]) == ("schlick", "refract"), lo.what
    exact, pairs = MS.shade_near_zero_pairs(T)
    assert all(sent[id(s)] == "degenerate" for s in exact)
    for lo, hi in pairs:
        assert (sent[id(lo)], sent[id(hi)]) == ("degenerate", "ball")
    assert {sent[id(s)] for s in MS.shade_clamp_items(T)} == {"tir", "schlick", "refract"}


@pytest.mark.parametrize("T", F, ids=IDS)
def test_one_bounce_in_the_sweep_scene(oracle, T):
    """op 26 on the camera rays of the sweep scene and on the rays their first bounce leaves (these start inside the glass): every
    sphere of the scene is hit, dielectrics on both faces, and a miss leaves the state alone"""
    flat, cam = MS.sweep_scene(T)
    W, H = 48, 27
    st = np.stack([oracle.rng_stream(SEED, p, 0) for p in range(W * H)])
    rays = np.zeros((W * H, 6))
    for j in range(W):
        for i in range(H):
            p = j * H + i
            rays[p], st[p] = oracle.get_ray(cam, (j + 0.5) / W, (i + 0.5) / H, st[p], T)
    hit_back = set()
    hit_any = set()
    misses = 0
    for bounce in range(2):
        y = run_unit(26, np.concatenate([st.view(np.float64), rays], 1), 12, T, flat=flat)
        keep = []
        for p in range(len(rays)):
            br, idx, out, s1, front = MS.shade_branch(flat, rays[p, :3], rays[p, 3:], st[p], T)
            assert int(y[p, 2]) == idx, (bounce, p)
            assert np.array_equal(y[p, :2].view(np.uint64), s1), (bounce, p, br)
            if idx < 0:
                misses += 1
                assert not y[p, 3:].any()
                continue
            _bits_equal(y[p, 3:12].astype(T), out, f"bounce {bounce} ray {p} sphere {idx} ({br})")
            hit_any.add(idx)
            if not front:
                hit_back.add(idx)
            keep.append((s1, _wide(out[:6])))
        st = np.stack([k[0] for k in keep])
        rays = np.stack([k[1] for k in keep])
    assert hit_any == set(range(MS.N_BASE)) and set(MS.DIELECTRICS) <= hit_back and misses > 0


# ---- render level -------------------------------------------------------------------------------------------------------------------------
def _scene(T, extra=0):
    flat, cam = MS.sweep_scene(T, extra)
    return flat, CamObj(cam)


def _second_camera(oracle, T):
    return CamObj(oracle.default_camera((-4, 1.2, 5), (0.5, 0.4, 0), (0, 1, 0), 45, 16 / 9, 0.0, 6.0, T))


def _ref(oracle, T, frame, extra=0, cam=None, seed=SEED, key="", flat=None):
    """oracle.render in the current numerics mode, computed once -> (img, segments)"""
    W, H, spp, nch, depth = frame
    k = (np.dtype(T).name, frame, extra, key, seed, oracle._default_numerics)
    if k not in _refs:
        f, c = _scene(T, extra)
        img, st = oracle.render(f if flat is None else flat, c if cam is None else cam, W, H, spp, T=T, max_depth=depth, seed=seed, n_chunks=nch)
        img.setflags(write=False)
        _refs[k] = (img, st["segments"])
    return _refs[k]


@pytest.mark.parametrize("frame", list(FRAMES), ids=list(FRAMES))
@pytest.mark.parametrize("flags", [0, 4, 1], ids=["matrix", "valu", "cull"])
@pytest.mark.parametrize("extra", [0, 24])
@pytest.mark.parametrize("T", F, ids=IDS)
def test_render_equals_the_oracle(oracle, T, extra, flags, frame):
    """one block (the caller's order) and, with the 24 extra spheres, two blocks (the plain layout and group cull reorder the rows)"""
    W, H, spp, nch, depth = FRAMES[frame]
    flat, cam = _scene(T, extra)
    ref, seg = _ref(oracle, T, FRAMES[frame], extra)
    img, st = PA.single(flat, cam, T, W, H, spp, depth, SEED, n_chunks=nch, flags=flags)
    _bits_equal(img, ref, f"flags {flags}")
    assert st.segments == seg and st.samples == W * H * spp


@pytest.mark.usefixtures("numerics")
@pytest.mark.parametrize("frame", list(FRAMES), ids=list(FRAMES))
@pytest.mark.parametrize("T", F, ids=IDS)
def test_numerics_modes(oracle, T, frame):
    W, H, spp, nch, depth = FRAMES[frame]
    flat, cam = _scene(T)
    ref, seg = _ref(oracle, T, FRAMES[frame])
    img, st = PA.single(flat, cam, T, W, H, spp, depth, SEED, n_chunks=nch)
    _bits_equal(img, ref, "one-shot")
    assert st.segments == seg


@pytest.mark.parametrize("T", F, ids=IDS)
def test_batch_of_two_cameras(oracle, T):
    W, H, spp, nch, depth = FRAME_A
    flat, cam = _scene(T)
    cams, seeds = [cam, _second_camera(oracle, T)], [SEED, SEED + 6]
    imgs, st = B.batch(flat, cams, seeds, T, W, H, spp, depth, n_chunks=nch)
    seg = 0
    for v in range(2):
        ref, s = _ref(oracle, T, FRAME_A, cam=cams[v], seed=seeds[v], key=f"view {v}")
        _bits_equal(imgs[v], ref, f"view {v}")
        seg += s
    assert st.segments == seg
    assert (FR.bits(np.ascontiguousarray(imgs[0])) != FR.bits(np.ascontiguousarray(imgs[1]))).any()


@pytest.mark.parametrize("T", F, ids=IDS)
def test_progressive_render_in_two_uneven_passes(oracle, T):
    W, H, spp, nch, depth = FRAME_A
    flat, cam = _scene(T)
    ref, oseg = _ref(oracle, T, FRAME_A)
    a = PA.Acc(flat, cam, T, W, H, spp, depth, SEED, n_chunks=nch)
    try:
        seg = a.add_ok(1, 3).segments + a.add_ok(0, 1).segments
        assert a.info()["complete"] == 1
        _bits_equal(a.resolve(), ref, "chunks [1, 4) then [0, 1)")
        assert seg == oseg
    finally:
        a.close()


@pytest.mark.parametrize("T", F, ids=IDS)
def test_adaptive_render_with_an_unreachable_tolerance(oracle, T):
    W, H, spp, nch, depth = FRAME_A
    flat, cam = _scene(T)
    ref, oseg = _ref(oracle, T, FRAME_A)
    a = Ad(flat, cam, T, W, H, spp, depth, SEED, n_chunks=nch, min_chunks=2, check_chunks=2)
    try:
        a.run_ok(UNREACHABLE)
        assert (a.chunks() == a.n_chunks).all()
        _bits_equal(a.resolve(), ref, "adaptive")
        assert a.stats().segments == oseg
    finally:
        a.close()


@pytest.mark.parametrize("flags", [0, 4], ids=["matrix", "valu"])
@pytest.mark.parametrize("T", F, ids=IDS)
def test_feature_pass_equals_the_witness(oracle, T, flags):
    """a dielectric first hit reports albedo (1, 1, 1), not the constants that stand in the albedo slots of its material row"""
    W, H, spp, nch, _ = FRAME_B
    flat, cam = MS.sweep_scene(T)
    it = FR.items(flat, cam, W, H, spp, nch, SEED, T, key="material sweep")
    ref, poisoned = FR.resolve(it, T)
    assert not poisoned.any()
    glass = (it["kind"] == MS.DIELECTRIC).all(axis=2)
    assert glass.sum() >= 50 and (FR.bits(ref[glass][:, :3]) == FR.bits(np.ones(3, T))).all()
    raw, st = GF.features_host(flat, cam, T, W, H, spp, nch, (0, it["N"]), seed=SEED, flags=flags)
    raw = np.ascontiguousarray(raw)
    assert (FR.bits(raw[glass][:, :3]) == FR.bits(np.ones(3, T))).all()
    GF._assert_same_bits(raw, ref, f"flags {flags}")
    GF._assert_stats(st, W, H, it["N"], MS.N_BASE, it["N"])


@pytest.mark.parametrize("flags", [0, 4, 1], ids=["matrix", "valu", "cull"])
def test_in_front_of_a_field_read_from_global_memory(oracle, flags):
    """1618 Float32 spheres: past the LDS scene copy (tests/big_scenes.py), the material rows come from global memory; a one-shot render
    and a progressive one in two passes"""
    T = np.float32
    W, H, spp, nch, depth = FRAME_A
    flat, cam = MS.in_front_of_a_field(T)
    assert flat["n"] > 1528
    ref, oseg = _ref(oracle, T, FRAME_A, flat=flat, key="field")
    base, _ = _ref(oracle, T, FRAME_A)
    assert (FR.bits(np.ascontiguousarray(ref)) != FR.bits(np.ascontiguousarray(base))).any()
    img, st = PA.single(flat, CamObj(cam), T, W, H, spp, depth, SEED, n_chunks=nch, flags=flags)
    _bits_equal(img, ref, "one-shot")
    assert st.segments == oseg
    a = PA.Acc(flat, CamObj(cam), T, W, H, spp, depth, SEED, n_chunks=nch)
    try:
        seg = a.add_ok(3, 1, flags=flags).segments + a.add_ok(0, 3, flags=flags).segments
        _bits_equal(a.resolve(), ref, "two passes")
        assert seg == oseg
    finally:
        a.close()


@needs_pool
@pytest.mark.parametrize("frame", list(FRAMES), ids=list(FRAMES))
def test_ray_pool_equals_the_oracle(oracle, frame):
    T = np.float32
    W, H, spp, nch, depth = FRAMES[frame]
    flat, cam = _scene(T)
    ref, seg = _ref(oracle, T, FRAMES[frame])
    img, st = PA.single(flat, cam, T, W, H, spp, depth, SEED, n_chunks=nch, flags=FLAG_POOL)
    _bits_equal(img, ref, "ray pool")
    assert st.segments == seg and st.block_threads == 1024
