"""The kernel instances that read the scene from global memory (LDS_SCENE = false: scenes of more than 1528 Float32 / 760 Float64 spheres,
csrc/rtw_launch.hip) behind the batched, progressive, adaptive, batched-progressive, batched-adaptive and feature entry points.  The
scenes, cameras and the table of instances are tests/big_scenes.py (CASES: every test here iterates its rows, and the probe at the end
checks in a fresh process that each row's launch reported the instance the row names).  The reference is the CPU oracle rendering the
same flat scene; where a GPU single-view call is compared as well (the exported state of a batch's accumulators) it comes on top of
the oracle.  Frames are 40 x 22 (ragged tiles), depth 8, unless said otherwise.  Every comparison is on the bits.  Tolerance: NONE."""
import os
import subprocess
import sys

import numpy as np
import pytest

import big_scenes as BS
import features_ref as FR
import test_gpu_accum as PA
import test_gpu_accum_batch as AB
import test_gpu_batch as B
import test_gpu_features as F
from test_gpu_adaptive import Ad, _same, all_samples, oracle_words, rule_chunks

pytestmark = pytest.mark.gpu

W, H, DEPTH = 40, 22, 8
_refs = {}


def _oracle_render(oracle, T, n, view, width, height, spp, n_chunks, seed=None, flat=None, key=""):
    """oracle.render of big_scenes.scene(T, n) through camera `view` in the current numerics mode, computed once -> (img, segments)"""
    seed = BS.VIEW_SEEDS[view] if seed is None else seed
    k = (np.dtype(T).name, n, view, width, height, spp, n_chunks, seed, key, oracle._default_numerics)
    if k not in _refs:
        img, st = oracle.render(BS.scene(T, n) if flat is None else flat, BS.cameras(T)[view], width, height, spp, T=T, max_depth=DEPTH, seed=seed,
                                n_chunks=n_chunks)
        img.setflags(write=False)
        _refs[k] = (img, st["segments"])
    return _refs[k]


def _assert_image(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    bad = FR.bits(got) != FR.bits(ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} channels differ from the oracle; first at {np.argwhere(bad)[:4].tolist()}"


# ---- a. batch: three views in one launch, in every numerics mode (a global instance takes the mode at run time) --------------------------
@pytest.mark.usefixtures("numerics")
@pytest.mark.parametrize("case", BS.cases("batch"))
def test_batch_views_equal_the_oracle(oracle, case):
    T, n = case.T, case.n
    imgs, st = B.batch(BS.scene(T), BS.cameras(T), list(BS.VIEW_SEEDS), T, W, H, 4, DEPTH, n_chunks=4, flags=case.flags)
    seg = 0
    for v in range(3):
        ref, s = _oracle_render(oracle, T, n, v, W, H, 4, 4)
        _assert_image(imgs[v], ref, f"view {v}")
        seg += s
    assert st.segments == seg
    assert st.sphere_tests == seg * n
    assert st.samples == 3 * W * H * 4


# ---- g. the tie and the hollow sphere are in the picture ----------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BS.FLAGS)
@pytest.mark.parametrize("T", BS.PRECISIONS, ids=["f32", "f64"])
def test_exchanging_the_albedos_of_the_coincident_pair_changes_the_image_as_the_oracle_says(oracle, T, flags):
    """the one-shot render of the batch test's first view: the later sphere of the pair wins the tie, so with the two albedos exchanged
    the oracle's image is another one, and the GPU's image changes with it (likewise with the hollow of the glass sphere filled)"""
    n, cam = BS.BIG[T], BS.cameras(T)[0]
    ref, seg = _oracle_render(oracle, T, n, 0, W, H, 4, 4)
    img, st = PA.single(BS.scene(T), cam, T, W, H, 4, DEPTH, BS.VIEW_SEEDS[0], n_chunks=4, flags=flags)
    _assert_image(img, ref, "as built")
    assert st.segments == seg
    for name, change in (("swapped", BS.swapped_pair), ("solid", BS.solid_glass)):
        flat = change(BS.scene(T))
        other, _ = _oracle_render(oracle, T, n, 0, W, H, 4, 4, flat=flat, key=name)
        assert (FR.bits(other) != FR.bits(ref)).any(), name
        got, _ = PA.single(flat, cam, T, W, H, 4, DEPTH, BS.VIEW_SEEDS[0], n_chunks=4, flags=flags)
        _assert_image(got, other, name)


# ---- b. progressive -------------------------------------------------------------------------------------------------------------------
def _passes(a, ranges, flags):
    seg = 0
    for begin, count in ranges:
        seg += a.add_ok(begin, count, flags=flags).segments
    return seg


@pytest.mark.parametrize("case", BS.cases("accum"))
def test_progressive_passes_equal_the_oracle(oracle, case):
    """8 chunks of one sample added as [5, 8), [0, 2), [2, 5); then 8 samples in 3 chunks of 3 (the last one short) added as [1, 3), [0, 1)"""
    T, n = case.T, case.n
    flat, cam = BS.scene(T), BS.cameras(T)[0]
    for n_chunks, eff, ranges in ((8, (8, 1), ((5, 3), (0, 2), (2, 3))), (3, (3, 3), ((1, 2), (0, 1)))):
        a = PA.Acc(flat, cam, T, W, H, 8, DEPTH, BS.VIEW_SEEDS[0], n_chunks=n_chunks)
        try:
            assert (a.n_chunks, a.chunk_spp) == eff
            seg = _passes(a, ranges, case.flags)
            ref, oseg = _oracle_render(oracle, T, n, 0, W, H, 8, n_chunks)
            assert a.info()["complete"] == 1 and a.info()["samples_done"] == 8
            _assert_image(a.resolve(), ref, f"n_chunks {n_chunks}")
            assert seg == oseg
        finally:
            a.close()


SW, SH = 16, 9          # the frame whose every sample the oracle lists


def _small_words(oracle, T):
    """the accumulator words of the 16 x 9 frame after all 8 one-sample chunks, from the oracle's samples; computed once"""
    k = ("words", np.dtype(T).name)
    if k not in _refs:
        samples = all_samples(oracle, BS.scene(T), BS.cameras(T)[0], T, SW, SH, 8, DEPTH, BS.VIEW_SEEDS[0], 8)
        w = oracle_words(samples, 1, [8])[8]
        w.setflags(write=False)
        _refs[k] = w
    return _refs[k]


@pytest.mark.parametrize("case", BS.cases("accum"))
def test_progressive_words_are_the_oracles_exact_sums(oracle, case):
    T = case.T
    a = PA.Acc(BS.scene(T), BS.cameras(T)[0], T, SW, SH, 8, DEPTH, BS.VIEW_SEEDS[0], n_chunks=8)
    try:
        _passes(a, ((5, 3), (0, 2), (2, 3)), case.flags)
        w = a.words()
        assert np.array_equal(w[..., :7], _small_words(oracle, T)[..., :7])     # the 128-bit sums and the poison count
        assert w[..., :6].any() and not w[..., 7].any()             # (word 7, the half difference, is an adaptive render's: a plain accumulator reads 0)
    finally:
        a.close()


# ---- c. adaptive ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=BS.PRECISIONS, ids=["f32", "f64"])
def adaptive(request, oracle):
    with oracle.numerics("reference"):
        return BS.adaptive_case(oracle, request.param)


def _ad(case, view=0, seed=BS.AD_SEED):
    T = case["T"]
    return Ad(case["flat"], BS.cameras(T)[view], T, BS.AD_W, BS.AD_H, BS.AD_SPP, BS.AD_DEPTH, seed, n_chunks=BS.AD_SPP, floor=BS.AD_FLOOR,
              min_chunks=BS.AD_CHECKS[0], check_chunks=BS.AD_CHECKS[1] - BS.AD_CHECKS[0])


def _expected_chunks(case, tol):
    return rule_chunks(case["words_at"], BS.AD_CHECKS, BS.AD_SPP, 1, BS.AD_W, BS.AD_H, tol, BS.AD_FLOOR)


def _assert_adaptive_state_is_the_oracles(oracle, case, a, tol, what):
    """C_t is the rule's on the oracle's words; every tile's words (word 7, the half difference, included) are the oracle's after C_t
    chunks; every tile of the resolved image is the oracle's render of that prefix"""
    T, n = case["T"], case["flat"]["n"]
    expect = _expected_chunks(case, tol)
    ct = a.chunks()
    assert np.array_equal(ct, expect), (what, ct.tolist(), expect.tolist())
    w, img = a.words(), a.resolve()
    assert (w[..., 7].view(np.int64) != 0).any()
    for c in sorted(set(int(x) for x in ct)):
        ref, _ = _oracle_render(oracle, T, n, 0, BS.AD_W, BS.AD_H, c, c, seed=BS.AD_SEED)
        for t in np.nonzero(ct == c)[0]:
            m = a.tile_mask(t)
            assert np.array_equal(w[m][:, 7], case["words_at"][c][m][:, 7]), (what, "word 7", c, int(t))
            assert np.array_equal(w[m], case["words_at"][c][m]), (what, "words", c, int(t))
            assert _same(img[m], ref[m]), (what, "image", c, int(t))
    ai = a.ainfo()
    assert ai["tiles_converged"] == (expect < BS.AD_SPP).sum() and ai["tiles_at_cap"] == (expect == BS.AD_SPP).sum()
    assert ai["samples"] == sum(a.npix(t) * int(ct[t]) for t in range(ct.size))
    return ct, w, img


@pytest.mark.parametrize("flags", BS.FLAGS)
def test_adaptive_decisions_words_and_tiles_are_the_oracles(oracle, adaptive, flags):
    case = adaptive
    tol = case["tol"]
    first, later, never = BS.stop_groups(case["ratios"], tol)
    assert first.sum() >= 5 and later.sum() >= 5 and never.sum() >= 5, (first.sum(), later.sum(), never.sum())
    got = []
    for jp in (0, 1):
        a = _ad(case)
        try:
            a.run_ok(tol, flags=flags, job_pixels=jp)
            ct, w, img = _assert_adaptive_state_is_the_oracles(oracle, case, a, tol, f"flags {flags} job_pixels {jp}")
            assert a.ainfo()["samples"] == a.stats().samples
            got.append((ct.copy(), w.copy(), img.copy()))
        finally:
            a.close()
    assert np.array_equal(ct, np.where(first, BS.AD_CHECKS[0], ct)) and (ct[never] == BS.AD_SPP).all()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]) and _same(got[0][2], got[1][2])


# ---- d. batched progressive and batched adaptive ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BS.cases("batch_accum"))
def test_batched_progressive_passes_equal_the_single_view_calls_and_the_oracle(oracle, case):
    """three views, two uneven passes ([3, 8) then [0, 3)) of 8 one-sample chunks"""
    T, n = case.T, case.n
    flat, cams = BS.scene(T), BS.cameras(T)

    def views(width, height):
        return [Ad(flat, cams[v], T, width, height, 8, DEPTH, BS.VIEW_SEEDS[v], n_chunks=8) for v in range(3)]
    b, s = views(W, H), views(W, H)
    try:
        seg_b = 0
        for begin, count in ((3, 5), (0, 3)):
            AB.ok(AB.batch_accum(b, begin, count, flags=case.flags), b[0])
            st = b[0].stats()
            assert st.samples == 3 * W * H * count
            seg_b += st.segments
        seg_o = 0
        for v in range(3):
            assert s[v].add(3, 5) == 0 and s[v].add(0, 3) == 0
            AB.assert_same_state(AB.state(b[v], False), AB.state(s[v], False), v)
            ref, oseg = _oracle_render(oracle, T, n, v, W, H, 8, 8)
            _assert_image(b[v].resolve(), ref, f"view {v}")
            seg_o += oseg
        assert seg_b == seg_o
    finally:
        AB.close(b, s)
    b = views(SW, SH)
    try:
        for begin, count in ((3, 5), (0, 3)):
            AB.ok(AB.batch_accum(b, begin, count, flags=case.flags), b[0])
        assert np.array_equal(b[0].words()[..., :7], _small_words(oracle, T)[..., :7]) and not b[0].words()[..., 7].any()
    finally:
        AB.close(b)


@pytest.mark.parametrize("flags", BS.FLAGS)
def test_batched_adaptive_run_and_refinement_equal_the_single_view_calls_and_the_oracle(oracle, adaptive, flags):
    """three views (view 0 is the adaptive case above) at its tolerance, then refined to 0.8 x that"""
    case = adaptive
    tols = (case["tol"], 0.8 * case["tol"])
    seeds = (BS.AD_SEED,) + BS.VIEW_SEEDS[1:]
    b, s = [_ad(case, v, seeds[v]) for v in range(3)], [_ad(case, v, seeds[v]) for v in range(3)]
    try:
        for tol in tols:
            AB.ok(AB.batch_adapt(b, tol, flags=flags), b[0])
            st = b[0].stats()
            seg = smp = 0
            for v in range(3):
                s[v].run_ok(tol)
                seg += s[v].stats().segments
                smp += s[v].stats().samples
                AB.assert_same_state(AB.state(b[v], True), AB.state(s[v], True), (tol, v))
            assert (st.segments, st.samples) == (seg, smp), tol
            _assert_adaptive_state_is_the_oracles(oracle, case, b[0], tol, f"flags {flags} tol {tol}")
        coarse, fine = _expected_chunks(case, tols[0]), _expected_chunks(case, tols[1])
        assert (fine >= coarse).all() and (fine > coarse).any()            # (the refinement is one: some tile goes on)
    finally:
        AB.close(b, s)


# ---- e. features ----------------------------------------------------------------------------------------------------------------------
FEATURE_VIEWS = (0, 2)      # cfg2's camera; t_default_cam, which stands ON the ground sphere: every one of its rays has a root at t ~ 0 that tmin = 1e-4 rejects


def _feature_items(T, view):
    cam = BS.camera_dict(BS.cameras(T)[view])
    return cam, FR.items(BS.scene(T), cam, W, H, 4, 4, BS.VIEW_SEEDS[view], T, key=f"big_scene view {view}")


@pytest.mark.parametrize("case", BS.cases("features_host") + BS.cases("features_device"))
def test_feature_words_of_a_chunk_range_equal_the_witness(oracle, case):
    """the chunks [1, 3) of 4, through two cameras"""
    T, n = case.T, case.n
    for view in FEATURE_VIEWS:
        with oracle.numerics("reference"):
            cam, it = _feature_items(T, view)
            ref, poisoned = FR.resolve(it, T, (1, 2))
        assert not poisoned.any() and (ref[..., 7] > 0).any() and (ref[..., 7] == 0).any()
        if case.entry == "features_host":
            raw, st = F.features_host(BS.scene(T), cam, T, W, H, 4, 4, (1, 2), seed=BS.VIEW_SEEDS[view], flags=case.flags)
        else:
            with F.DeviceScene(BS.scene(T), T) as ds:
                raw, st = ds.features(cam, W, H, 4, 4, (1, 2), seed=BS.VIEW_SEEDS[view], flags=case.flags)
        F._assert_same_bits(np.ascontiguousarray(raw), ref, f"{case.entry} flags {case.flags} view {view}")
        F._assert_stats(st, W, H, 2, n, 4)


# ---- f. the boundary: the largest scene that is staged in LDS and the smallest that is not ---------------------------------------------------
@pytest.mark.parametrize("case", BS.boundary_cases())
def test_boundary_sizes_equal_the_oracle(oracle, case):
    """a one-shot render, and a progressive render in two passes ([2, 4) then [0, 2))"""
    T, n = case.T, case.n
    flat, cam = BS.scene(T, n), BS.cameras(T)[0]
    ref, oseg = _oracle_render(oracle, T, n, 0, W, H, 4, 4)
    if case.entry == "render":
        img, st = PA.single(flat, cam, T, W, H, 4, DEPTH, BS.VIEW_SEEDS[0], n_chunks=4, flags=case.flags)
        _assert_image(img, ref, "one-shot")
        assert st.segments == oseg and st.sphere_tests == oseg * n
    else:
        a = PA.Acc(flat, cam, T, W, H, 4, DEPTH, BS.VIEW_SEEDS[0], n_chunks=4)
        try:
            seg = _passes(a, ((2, 2), (0, 2)), case.flags)
            _assert_image(a.resolve(), ref, "two passes")
            assert seg == oseg
        finally:
            a.close()


# ---- the probe: the instances were really reached -------------------------------------------------------------------------------------------
_PROBE = """
import sys
sys.path[:0] = [{tests!r}, {root!r}, {oracle!r}]
import torch
torch.cuda.init()                       # (two HIP runtimes in one process: torch's goes first, tests/conftest.py)
import big_scenes as BS
for k, case in enumerate(BS.CASES):
    print("@case", k, file=sys.stderr, flush=True)
    BS.launch(case)
print("walked", len(BS.CASES))
"""


def test_every_row_of_the_table_reaches_its_instance():
    """The environment aids are read once per process, so a fresh process walks the table (8 x 5 pixels, 2 spp) under RTW_DEBUG: every
    launch of a row reports the row's instance, together the rows reach all 40 global-scene trace instances with BATCH or ACCUM and the
    4 global-scene feature instances, and lds_scene flips between the two sizes of each boundary pair in the plain scans."""
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    code = _PROBE.format(tests=tests, root=root, oracle=os.path.join(root, "oracle"))
    env = dict(os.environ, RTW_ENABLE_TEST_AIDS="1", RTW_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert f"walked {len(BS.CASES)}" in r.stdout
    sections = r.stderr.split("@case ")[1:]
    assert len(sections) == len(BS.CASES)
    reached, seen = set(), {}
    for k, (case, text) in enumerate(zip(BS.CASES, sections)):
        assert int(text.split()[0]) == k
        lines = BS.parse_instance_lines(text)
        assert lines, (case, text[-500:])
        for inst, lds_bytes, blocks_per_cu in lines:
            assert BS.matches(inst, case.expect), (case, inst)
            assert lds_bytes > 0 and (inst.kernel == "features" or blocks_per_cu >= 1)
            reached.add(inst)
            seen.setdefault((case.entry, BS._prec(case.T), case.flags), {}).setdefault(case.n, set()).add(inst.lds_scene)
    want = BS.global_instances()
    cull = {k: v for k, v in seen.items() if k[0] == "render" and k[2] & 1}
    print(f"global-scene instances reached: {len(want & reached)} of {len(want)}; group cull at the boundary sizes, lds_scene: {cull}")
    assert not want - reached, sorted(want - reached)
    for T in BS.PRECISIONS:
        lo, hi = BS.BOUNDARY[T]
        for flags in (0, 4):
            for entry in ("render", "accum"):
                by_n = seen[(entry, BS._prec(T), flags)]
                assert by_n[lo] == {1} and by_n[hi] == {0}, (entry, T, flags, by_n)
