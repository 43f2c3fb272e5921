"""The candidate lists of the closest-hit scans at and beyond their capacities: the five places where a full list is resolved in the
middle of a scan (csrc/rtw_scan.hpp RTW_FLUSH_A .. E), pinned by the hand-made waves of tests/list_cases.py (checked on the CPU by
tests/test_list_cases.py) and by small renders of a nest of spheres in which every ray has ~200 candidates.

Unit ops 32 - 35 are the candidate sinks of ops 17 - 20 with one more slot per ray, a raw uint64 of four 16-bit counts: how often a
list was resolved early during that ray's scan -- bits 0-15 A, 16-31 B, 32-47 C (ops 34, 35: hit_world_mfma), bits 48-63 D (op 32:
hit_world) or E (op 33: hit_world_cull, the lane's own count; A - D are the wave's and stand in every live row alike).

Asserted per case, precision and numerics mode: index and t of every lane equal oracle.hit_world_batch on the bits (ops 8, 10, 11, 13,
14); the candidate sets equal the design for the plain ops and cover the oracle's hits for the cull ops; the counts of early resolves
are EXACTLY those of the rules restated in list_cases (0 against 1 on the boundary pairs) and at least the pigeonhole bounds of the
heavy case -- for the cull ops from the device order that op 28 reports; the winner of a tie is the last copy of the caller's list."""
import collections
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import list_cases as LC
from test_gpu_filters import centres, oracle_sets, run_sink
from test_gpu_units import run_unit

pytestmark = pytest.mark.gpu
FLUSH = {10: 32, 11: 33, 13: 34, 14: 35}
F = [np.float32, np.float64]


def run_flush(op, flat, o, d, tmin, tmax, T):
    """-> ok, mf_sc, candidates [m, 512], in-lane [m, 512], counts [m] dicts of A, B, C, DE"""
    m = len(o)
    x = np.concatenate([o, d, np.full((m, 1), float(tmin)), np.broadcast_to(np.asarray(tmax, np.float64), (m,))[:, None]], 1)
    y = run_unit(FLUSH[op], x, 19, T, flat=flat)
    bits = lambda a: np.unpackbits(np.ascontiguousarray(a).view(np.uint64).astype("<u8").view(np.uint8), bitorder="little").reshape(m, 512)
    w = np.ascontiguousarray(y[:, 18]).view(np.uint64)
    counts = {k: ((w >> np.uint64(16 * f)) & np.uint64(0xffff)).astype(np.int64) for f, k in enumerate(("A", "B", "C", "DE"))}
    return y[:, 0] != 0, y[:, 1], bits(y[:, 2:10]).astype(bool), bits(y[:, 10:18]).astype(bool), counts


def cull_layout(flat, T):
    """op 28 -> (the caller's index per device position or -1, in-lane per position)"""
    import exact_vote as V
    lay = V.layout_of(run_unit(28, np.zeros((1024, 1)), 4, T, flat=flat))
    return lay.idx, lay.inlane


def device_rows(inc, idx):
    """[count, n] in the caller's order -> [64, positions] in the device order"""
    out = np.zeros((64, len(idx)), bool)
    live = idx >= 0
    out[:len(inc)][:, live] = inc[:, idx[live]]
    return out


@pytest.mark.usefixtures("numerics")
@pytest.mark.parametrize("count", LC.COUNTS)
@pytest.mark.parametrize("T", F, ids=["f32", "f64"])
def test_hand_made_waves(oracle, T, count, numerics):
    f32 = T is np.float32
    census = collections.defaultdict(collections.Counter)
    for case in LC.cases(count):
        flat = case.flat(T)
        o, d = case.rays(T)
        n, inc = case.n, case.incidence()
        tmax = np.full(count, np.inf)
        tag = (case.name, np.dtype(T).name, count, numerics)
        ref_idx, ref_t = oracle.hit_world_batch(flat, np.concatenate([o, d], 1).astype(T), T(LC.TMIN), np.inf, T)
        _, dset, hset = oracle_sets(oracle, flat, o, d, LC.TMIN, tmax, T)
        assert np.array_equal(dset, inc), tag
        copies = case.copies(ref_idx) if case.tie else None
        if case.tie:
            assert all(ref_idx[l] == cp[-1] for l, cp in enumerate(copies) if len(cp) >= 2), tag
        x = np.concatenate([o, d, np.full((count, 1), float(T(LC.TMIN))), np.full((count, 1), np.inf)], 1)
        want, w13, w10 = LC.plain_counts(case)
        huge = LC.huge_of(case.r)
        idx, inl_pos = cull_layout(flat, T)
        pos_of = {int(i): p for p, i in enumerate(idx) if i >= 0}
        assert sorted(pos_of) == list(range(n)), tag
        for op in (8, 10, 11, 13, 14):
            y = run_unit(op, x, 9, T, flat=flat)
            wrong = (y[:, 0].astype(np.int64) != ref_idx) | ((ref_idx >= 0) & (y[:, 1] != ref_t.astype(np.float64)))
            assert not wrong.any(), (tag, op, np.flatnonzero(wrong)[:5], y[wrong][:3, :2], ref_idx[wrong][:3], ref_t[wrong][:3])
        for op in (10, 11, 13, 14):
            ok, sc, cand, inl, cnt = run_flush(op, flat, o, d, float(T(LC.TMIN)), tmax, T)
            ok0, sc0, cand0, inl0 = run_sink(op, flat, o, d, float(T(LC.TMIN)), tmax, T)
            assert np.array_equal(cand, cand0) and np.array_equal(inl, inl0) and np.array_equal(ok, ok0), (tag, op)      # the counter changes nothing else
            assert ok.all(), (tag, op)
            have = (cand | inl)[:, :n]
            assert not (cand | inl)[:, n:].any(), (tag, op)
            if op in (10, 13):
                assert np.array_equal(have, inc), (tag, op, [(int(a), int(b)) for a, b in zip(*np.nonzero(have != inc))][:5])
                assert sorted(set(np.nonzero(inl)[1])) == (sorted(huge) if op == 13 else []), (tag, op)
            else:
                assert not (hset & ~have).any() and not (have & ~inc).any(), (tag, op)
            for k in cnt:
                if not (op == 11 and k == "DE"):
                    assert (cnt[k] == cnt[k][0]).all(), (tag, op, k, cnt[k])                 # the wave's counts: every live row alike
            got = {k: int(v[0]) for k, v in cnt.items()}
            if op == 10:
                assert got == dict(A=0, B=0, C=0, DE=want["D"]), (tag, op, got, want)
                assert want["D"] >= case.at_least.get("D", 0)
            elif op == 13:
                assert got == dict(A=want["A"], B=0, C=want["C"], DE=0), (tag, op, got, want)
                assert want["A"] >= case.at_least.get("A", 0) and want["C"] >= case.at_least.get("C", 0)
            elif op == 11:
                big = set(LC.big_of(case.r))
                order = [sorted((int(i) for i in np.flatnonzero(inc[l])), key=lambda i: (i not in big, pos_of[i])) for l in range(count)]
                E = LC.model_cull_valu(order)
                assert cnt["DE"].tolist() == E and got["A"] == got["B"] == got["C"] == 0, (tag, op, cnt["DE"].tolist(), E)
                assert min(E) >= case.at_least.get("E", 0)
                if case.tie:
                    when = {(l, i): k // LC.LIST_CAP for l in range(count) for k, i in enumerate(order[l])}
                    census[11].update(LC.classify_ties(case, copies, when))
            else:
                # the group cull on the matrix pipe: the same rules over the device order; in-lane: the huge spheres exactly, the rest of the list
                # (Float32: the BIG class when it fits) through the filter, in the layout's order
                inl_set = sorted(int(p) for p in np.flatnonzero(inl_pos))
                exact = [p for p in inl_set if int(idx[p]) in huge]
                filt = [p for p in inl_set if int(idx[p]) not in huge]
                assert len(exact) == len(huge) and (f32 or not filt), (tag, inl_set)
                A, B, C, when = LC.model_mfma(device_rows(inc, idx), exact=exact, inlane=filt)
                assert got == dict(A=A, B=B, C=C, DE=0), (tag, op, got, (A, B, C))
                assert A >= case.at_least.get("A", 0) and C >= case.at_least.get("C", 0)
                if case.name == "B_inlane_filter":
                    assert B == (1 if f32 else 0) and len(filt) == (4 if f32 else 0), (tag, B, filt)
                if case.tie:
                    census[14].update(LC.classify_ties(case, copies, when, key=lambda ray, i: (ray, pos_of[i])))
    # the cull ops' own order: copies either side of an early resolve in BOTH orders (list_cases.tie_many), and for the matrix pipe either side
    # of a C flush too
    print("tie arrangements in the cull layout's order, op 11:", dict(census[11]), " op 14:", dict(census[14]))
    for op in (11, 14):
        have = {(r_, o_) for r_, o_, f_ in census[op]}
        assert {("A", "aligned"), ("A", "opposed")} <= have, (op, dict(census[op]))
    assert {("C", "aligned"), ("C", "opposed")} <= {(r_, o_) for r_, o_, f_ in census[14]}, dict(census[14])


# ---- the kernels that ship: four waves side by side in the list area ------------------------------------------------------------------
W, H, SPP, DEPTH, N_NEST = 16, 9, 2, 8, 200
COPIES = (5, 101, N_NEST - 1)                     # the outermost sphere: a first, a middle and the last block of the caller's list


def nest(rtw, T, glass):
    """~200 spheres around the origin, radii 1.0 .. 1.4, centres jittered by <= 0.05 (all distinct), and an outermost one of radius 1.5 AT
    the origin three times over -- caller's indices 5, 101 and 199, three materials.  The last copy is what every primary ray hits:
    Lambertian of an albedo of its own, or (`glass`) Dielectric, so that the next segments start INSIDE the nest."""
    rng = np.random.default_rng(41)
    s = rtw.HittableList()
    for i in range(N_NEST):
        alb = np.array(rng.uniform(0.2, 0.9, 3), T)
        if i in COPIES:
            mat = (rtw.Lambertian(np.array([0.9, 0.1, 0.1], T)), rtw.Metal(np.array([0.1, 0.9, 0.1], T), T(0.3)),
                   rtw.Dielectric(T(1.5)) if glass else rtw.Lambertian(np.array([0.1, 0.2, 0.9], T)))[COPIES.index(i)]
            s.append(rtw.Sphere(np.array([0, 0, 0], T), T(1.5), mat))
        else:
            c = np.array(rng.uniform(-0.05, 0.05, 3) / np.sqrt(3), T)
            mat = (rtw.Lambertian(alb), rtw.Metal(alb, T(rng.uniform(0, 0.4))), rtw.Dielectric(T(1.5)))[i % 3 if i % 7 else 0]
            s.append(rtw.Sphere(c, T(1.0 + 0.4 * i / N_NEST), mat))
    return s


def nest_camera(rtw, T, eye=(0, 0, 6)):
    return rtw.default_camera(eye, (0, 0, 0), (0, 1, 0), 8, 16 / 9, 0.0, 6.0, elem_type=T)          # the frame lies inside the innermost sphere's outline


def _sha(img):
    return hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest()


@pytest.mark.usefixtures("numerics")
@pytest.mark.parametrize("glass", [False, True], ids=["lambertian", "dielectric"])
@pytest.mark.parametrize("T", F, ids=["f32", "f64"])
def test_nest_renders(rtw, oracle, T, glass):
    import features_ref as FR
    from test_gpu_features import features_host, _assert_same_bits
    scene, cam = nest(rtw, T, glass), nest_camera(rtw, T)
    flat = rtw.flatten_scene(scene, T)
    cc, rr = centres(flat)
    assert len({tuple(c) for c in cc}) == N_NEST - 2 and not LC.big_of(rr) and not LC.huge_of(rr)
    ref, ost = oracle.render(flat, cam, W, H, SPP, T=T, max_depth=DEPTH, seed=3)
    for flags in (0, 1, 4, 5):
        img = rtw.render(scene, cam, W, SPP, depth=DEPTH, seed=3, group_cull=bool(flags & 1), scan_valu=bool(flags & 4))
        assert np.array_equal(img, ref), (flags, int((img != ref).sum()))
        assert rtw.last_stats()["segments"] == ost["segments"], flags
    # the last copy is in the picture: with its material given to the first copy the image is another one
    other = rtw.HittableList(scene)
    other[COPIES[0]], other[COPIES[2]] = scene[COPIES[2]], scene[COPIES[0]]
    assert not np.array_equal(ref, oracle.render(rtw.flatten_scene(other, T), cam, W, H, SPP, T=T, max_depth=DEPTH, seed=3)[0])
    # the feature pass, both scans with and without the group cull
    camd = {k: getattr(cam, k) for k in vars(cam)}
    it = FR.items(flat, camd, W, H, SPP, 0, 3, T)
    fref, poisoned = FR.resolve(it, T)
    assert not poisoned.any()
    for flags in (0, 1, 4, 5):
        raw, _ = features_host(flat, camd, T, W, H, SPP, 0, (0, it["N"]), seed=3, flags=flags)
        _assert_same_bits(np.ascontiguousarray(raw), fref, f"features flags={flags}")
    # one batch of two views and one progressive render in two passes equal the single calls
    cams = [cam, nest_camera(rtw, T, eye=(0.5, 0.3, 6))]
    for cull in (False, True):
        imgs = rtw.render_batch(scene, cams, W, SPP, depth=DEPTH, seed=[3, 4], group_cull=cull)
        assert np.array_equal(imgs[0], ref), cull
        ref1, _ = oracle.render(flat, cams[1], W, H, SPP, T=T, max_depth=DEPTH, seed=4)
        assert np.array_equal(imgs[1], ref1), cull
    with rtw.ProgressiveRenderer(scene, cam, W, SPP, depth=DEPTH, seed=3) as pr:
        pr.add(1)
        seg = pr.stats()["segments"]
        pr.add(SPP - 1)
        seg += pr.stats()["segments"]
        assert pr.done and np.array_equal(pr.image(), ref) and seg == ost["segments"]


@pytest.mark.usefixtures("numerics")
@pytest.mark.parametrize("T", F, ids=["f32", "f64"])
def test_nest_primary_rays_flush_every_list(rtw, oracle, T):
    """non-vacuity of the renders above: 64 primary rays of the frame's first tile (pixel centres, the pinhole camera: oracle.get_ray), one
    wave, through the counting sinks -- every ray takes every sphere, the lists are resolved early in every scan"""
    scene, cam = nest(rtw, T, False), nest_camera(rtw, T)
    flat = rtw.flatten_scene(scene, T)
    camd = {k: getattr(cam, k) for k in vars(cam)}
    rays = np.array([oracle.get_ray(camd, (i + 0.5) / W, (j + 0.5) / H, [1, 2], T)[0] for j in range(8) for i in range(8)], np.float64)
    o, d = rays[:, :3], rays[:, 3:]
    tmax = np.full(64, np.inf)
    _, dset, hset = oracle_sets(oracle, flat, o, d, 1e-4, tmax, T)
    assert dset.all()
    ref_idx, _ = oracle.hit_world_batch(flat, rays.astype(T), T(1e-4), np.inf, T)
    assert (ref_idx == COPIES[2]).all()
    for op in (10, 11, 13, 14):
        ok, sc, cand, inl, cnt = run_flush(op, flat, o, d, float(T(1e-4)), tmax, T)
        assert ok.all() and cand[:, :N_NEST].all(), op
        if op in (13, 14):
            assert (cnt["A"] > 0).all() and (cnt["C"] > 0).all(), (op, cnt)
        else:
            assert (cnt["DE"] > 0).all(), (op, cnt)


_AID = """
import hashlib, sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import numpy as np, rtw_amd as R
from test_gpu_list_caps import nest, nest_camera, W, SPP, DEPTH
for T in (np.float32, np.float64):
    for glass in (False, True):
        img = R.render(nest(R, T, glass), nest_camera(R, T), W, SPP, depth=DEPTH, seed=3)
        print("sha", np.dtype(T).name, glass, hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest())
"""


def test_nest_in_the_callers_order_and_in_the_plain_layouts(rtw, oracle):
    """the plain matrix-pipe scan with its own sphere order (ties by the orig[] word of the key) and, in a fresh process with the
    caller-order aid of test_gpu_plain_layout.py, in the caller's order: the same images, which are the oracle's"""
    tests = os.path.dirname(os.path.abspath(__file__))
    want = []
    for T in F:
        for glass in (False, True):
            scene, cam = nest(rtw, T, glass), nest_camera(rtw, T)
            ref, _ = oracle.render(rtw.flatten_scene(scene, T), cam, W, H, SPP, T=T, max_depth=DEPTH, seed=3)
            want.append(f"sha {np.dtype(T).name} {glass} {_sha(ref)}")
    lays = {}
    for aid in ("", "caller"):
        env = dict(os.environ, RTW_ENABLE_TEST_AIDS="1", RTW_DEBUG="1", RTW_PLAIN_ORDER=aid)
        r = subprocess.run([sys.executable, "-c", _AID.format(tests=tests, root=os.path.dirname(tests))], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert [ln for ln in r.stdout.splitlines() if ln.startswith("sha")] == want, aid
        lays[aid] = [ln.split("layout: ")[1] for ln in r.stderr.splitlines() if "plain scan layout" in ln]
    assert all("its own order" in ln for ln in lays[""]) and all("the caller's order" in ln for ln in lays["caller"]) and len(lays[""]) == 4, lays
