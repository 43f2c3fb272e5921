"""Batched progressive and adaptive renders on the GPU (include/rtw_hip.h rtw_render_accum_batch_*, rtw_render_adaptive_batch_*): N views of
one scene, each with its own accumulator, every pass one launch.  The contract: accumulator v after a batched call is indistinguishable
from the same accumulator after the single-view call with cams[v] and seeds[v].  So every comparison here is the batch against the
single-view calls (tests/test_gpu_accum.py, tests/test_gpu_adaptive.py pin those to the oracle) on the same GPU, ON THE BITS: the words
(word 7 included), C_t, rtw_accum_info, rtw_accum_adaptive_info (rounds included), the ranges, the export blob, the resolve and the frames
of d_out.  Tolerance of the comparisons: NONE.

The shared Float32 case is the frame of tests/test_gpu_adaptive.py -- cfg2's scene at 48 x 27 (6 x 4 tiles, a ragged last row), 64 chunks of
one sample, depth 8, checkpoints 16 / 32 / 48, dark_floor 0.03 -- seen by three views: the golden camera with seed 7, t_cam2 with seed 18,
t_cam1 with seed 1234574.  On the CPU oracle's samples (numerics "reference") tolerance 0.1 stops 14 / 9 / 1 / 0, 5 / 14 / 3 / 2 and
12 / 11 / 1 / 0 tiles of the three views at 16 / 32 / 48 / 64 chunks (nearest ratio 1 % from the tolerance): the views differ, two finish
early and the last pass holds tiles of view 1 only.  0.08 (nearest ratio 0.16 % away; 10/7/6/1, 0/9/8/7, 8/12/3/1) is the refinement target,
0.2 stops every tile at 16.  What the tests need of this is asserted on the SINGLE-VIEW runs (test_the_single_view_runs_are_a_real_case).
The Float64 case: random_64x36_8spp_d50_f64's scene at 24 x 13 (3 x 2 tiles), 24 spp in 8 chunks of 3, checkpoints every 2 chunks, the golden
camera with seed 3 and t_cam2 with seed 4; tolerance 0.15 (oracle: C_t = [2,4,2,4,2,4] and [8,6,8,4,2,2], nearest ratio 4.9 % away),
refined to 0.1 ([2,8,2,8,2,6] and [8,8,8,6,6,2], 3.2 %)."""
import ctypes as C

import numpy as np
import pytest

from conftest import CamObj, load_golden
from test_gpu_adaptive import DEPTH, FLOOR, H27, SCANS, SPP, UNREACHABLE, W48, Ad, _image, _same, single

pytestmark = pytest.mark.gpu

SEEDS = (7, 18, 1234574)
TOL, TOL_FINE, TOL_LOOSE = 0.1, 0.08, 0.2


# ---- N views = N `Ad` objects (an accumulator each; a scene's binding is a hash of its content, so view 0's upload serves the batch) ----
def _params(views, flags=0, job_pixels=0, gamma=1):
    return views[0]._params(flags, job_pixels, gamma)


def _arrays(views, seeds, cams=None):
    a = views[0]
    cams = a.C.make_cameras(cams or [v.cam for v in views], a.T)
    sd = a.C.make_seeds([v.seed for v in views], len(views)) if seeds == "own" else seeds
    return cams, sd, a.C.make_handles([v.acc for v in views])


def batch_accum(views, begin, count, flags=0, job_pixels=0, d_out=None, seeds="own", gamma=1, cams=None):
    """rtw_render_accum_batch_* -> return code (cameras and seeds: the views' own unless given)"""
    a = views[0]
    cams, sd, accs = _arrays(views, seeds, cams)
    P = _params(views, flags, job_pixels, gamma)
    fn = a.L.rtw_render_accum_batch_f64 if a.T is np.float64 else a.L.rtw_render_accum_batch_f32
    return fn(a.scene, cams, len(views), sd, C.byref(P), begin, count, accs, C.c_void_p(d_out) if d_out else None, None)


def batch_adapt(views, tol, flags=0, job_pixels=0, d_out=None, seeds="own", gamma=1, floor=None, cams=None):
    """rtw_render_adaptive_batch_* -> return code (cameras and seeds: the views' own unless given)"""
    a = views[0]
    cams, sd, accs = _arrays(views, seeds, cams)
    P = _params(views, flags, job_pixels, gamma)
    A = a.C.Adaptive(tol, a.floor if floor is None else floor, a.min_chunks, a.check_chunks)
    fn = a.L.rtw_render_adaptive_batch_f64 if a.T is np.float64 else a.L.rtw_render_adaptive_batch_f32
    return fn(a.scene, cams, len(views), sd, C.byref(P), C.byref(A), accs, C.c_void_p(d_out) if d_out else None, None)


def ok(rc, a):
    a.C.check(rc)


def export(a):
    size = C.c_uint64()
    a.C.check(a.L.rtw_accum_export(a.acc, None, 0, C.byref(size)))
    buf = np.empty(size.value, np.uint8)
    a.C.check(a.L.rtw_accum_export(a.acc, buf.ctypes.data_as(C.c_void_p), size.value, C.byref(size)))
    return buf.tobytes()


def state(a, adaptive):
    """everything the C ABI says about an accumulator"""
    d = dict(words=a.words().copy(), info=a.info(), ranges=a.ranges(), resolve=a.resolve().copy())
    if adaptive:
        d.update(chunks=a.chunks().copy(), ainfo=a.ainfo())
    else:
        d.update(blob=export(a))
    return d


def assert_same_state(x, y, what=""):
    assert x.keys() == y.keys(), what
    for k in x:
        if isinstance(x[k], np.ndarray):
            assert _same(x[k], y[k]), (what, k)
        else:
            assert x[k] == y[k], (what, k, x[k], y[k])


def frames(d_img, views):
    a = views[0]
    n = a.width * a.height * 3
    flat = d_img.cpu().numpy()
    return [_image(flat[v * n:(v + 1) * n], a.width, a.height) for v in range(len(views))]


def close(*groups):
    for g in groups:
        for a in g:
            a.close()


class Case:
    def __init__(self, flat, cams, seeds, T, width, height, spp, depth, n_chunks, min_chunks, check_chunks):
        self.flat, self.cams, self.seeds, self.T = flat, cams, seeds, T
        self.width, self.height, self.spp, self.depth, self.n_chunks = width, height, spp, depth, n_chunks
        self.min_chunks, self.check_chunks = min_chunks, check_chunks

    def views(self, which=None, seeds=None, width=None, height=None):
        which = range(len(self.cams)) if which is None else which
        return [Ad(self.flat, self.cams[v], self.T, width or self.width, height or self.height, self.spp, self.depth,
                   (seeds or self.seeds)[v], n_chunks=self.n_chunks, min_chunks=self.min_chunks, check_chunks=self.check_chunks) for v in which]

    def single_adaptive(self, tols):
        """fresh single-view runs refined through `tols` -> ([state per view], summed segments of the last call, summed stats samples)"""
        vs = self.views()
        try:
            seg = smp = 0
            for tol in tols:
                seg = smp = 0
                for a in vs:
                    a.run_ok(tol)
                    seg += a.stats().segments
                    smp += a.stats().samples
            return [state(a, True) for a in vs], seg, smp
        finally:
            close(vs)


@pytest.fixture(scope="module")
def case32(rtw):
    g = load_golden("cfg2_random_320x180_64spp_d16_f32", numerics="reference")
    T = np.float32
    cams = [CamObj(g["cam"]), rtw.t_cam2(elem_type=T), rtw.t_cam1(elem_type=T)]
    return Case(g["flat"], cams, SEEDS, T, W48, H27, SPP, DEPTH, SPP, 16, 16)


@pytest.fixture(scope="module")
def case64(rtw):
    g = load_golden("random_64x36_8spp_d50_f64", numerics="reference")
    T = np.float64
    return Case(g["flat"], [CamObj(g["cam"]), rtw.t_cam2(elem_type=T)], (3, 4), T, 24, 13, 24, 8, 8, 2, 2)


@pytest.fixture(scope="module")
def singles32(case32):
    """the single-view adaptive runs of the shared case (default numerics and scan), computed once: fresh at 0.1 and fresh at 0.08"""
    return {TOL: case32.single_adaptive([TOL]), TOL_FINE: case32.single_adaptive([TOL_FINE])}


def test_the_single_view_runs_are_a_real_case(singles32, case64):
    """what the tests below rely on, asserted on the single-view runs: the views stop differently, every checkpoint and the cap occur, and
    exactly one view is still active at the last checkpoint (so the last batched pass holds tiles of one view only)"""
    ct = [s["chunks"] for s in singles32[TOL][0]]
    assert not np.array_equal(ct[0], ct[1]) and not np.array_equal(ct[0], ct[2]) and not np.array_equal(ct[1], ct[2])
    assert set(np.concatenate(ct)) == {16, 32, 48, 64}
    assert sum(1 for c in ct if (c > 48).any()) == 1
    assert len({s["ainfo"]["rounds"] for s in singles32[TOL][0]}) > 1                 # (the rounds differ between the views, too)
    fine = [s["chunks"] for s in singles32[TOL_FINE][0]]
    assert all((f >= c).all() for f, c in zip(fine, ct)) and any((f > c).any() for f, c in zip(fine, ct))
    ct64 = [s["chunks"] for s in case64.single_adaptive([0.15])[0]]
    assert not np.array_equal(ct64[0], ct64[1]) and len(set(np.concatenate(ct64))) >= 3


# ---- 1. a progressive partition in batches equals the single-view passes ---------------------------------------------------------
@pytest.mark.usefixtures("numerics")
def test_progressive_partition_in_batches_equals_the_single_view_passes(case32):
    import torch
    b, s = case32.views(), case32.views()
    try:
        n_px = W48 * H27
        d_img = torch.full((3 * n_px * 3,), -1.0, dtype=torch.float32, device="cuda:0")
        seg_b = 0
        for begin, count, flags, jp in ((0, 16, 0, 0), (40, 24, SCANS["valu"], 4), (16, 24, SCANS["cull"], 0)):
            ok(batch_accum(b, begin, count, flags, jp, d_out=d_img.data_ptr()), b[0])
            st = b[0].stats()
            assert st.samples == 3 * n_px * count, (begin, count)
            seg_b += st.segments
        torch.cuda.synchronize()
        out = frames(d_img, b)
        seg_s = 0
        for a in s:
            assert a.add(0, SPP) == 0
            seg_s += a.stats().segments
        assert seg_b == seg_s
        for v in range(3):
            assert_same_state(state(b[v], False), state(s[v], False), v)
            assert b[v].info()["complete"] == 1 and b[v].ranges() == [(0, SPP)] and not b[v].words()[..., 7].any()
            one = single(case32.flat, case32.cams[v], case32.T, W48, H27, SPP, DEPTH, SEEDS[v], n_chunks=SPP)
            assert _same(b[v].resolve(), one), v
            assert _same(out[v], one), v                            # the last pass completes every view: its d_out frame is the resolve
    finally:
        close(b, s)


# ---- 2. accumulators that hold different ranges ----------------------------------------------------------------------------------
def test_uneven_accumulators_divide_their_own_frames_and_a_refusal_touches_nothing(case32):
    import torch
    b, s = case32.views(), case32.views()
    try:
        assert b[0].add(0, 8) == 0
        d_img = torch.full((3 * W48 * H27 * 3,), -1.0, dtype=torch.float32, device="cuda:0")
        ok(batch_accum(b, 8, 16, d_out=d_img.data_ptr()), b[0])
        torch.cuda.synchronize()
        out = frames(d_img, b)
        assert [a.info()["samples_done"] for a in b] == [24, 16, 16]
        assert [a.ranges() for a in b] == [[(0, 24)], [(8, 24)], [(8, 24)]]
        assert s[0].add(0, 24) == 0 and s[1].add(8, 16) == 0 and s[2].add(8, 16) == 0
        for v in range(3):
            assert _same(out[v], b[v].resolve()), v
            assert_same_state(state(b[v], False), state(s[v], False), v)
        before = [a.words().copy() for a in b]
        assert batch_accum(b, 0, 16) == -2 and b"overlaps" in b[0].L.rtw_last_error()
        assert batch_accum(b, 20, 8) == -2 and batch_accum(b[1:], 4, 8) == -2      # (an overlap at the end; one that views 1 and 2 alone have)
        for v in range(3):
            assert np.array_equal(b[v].words(), before[v]) and b[v].info()["samples_done"] == (24, 16, 16)[v]
    finally:
        close(b, s)


# ---- 3. a fresh adaptive batch equals the single-view runs, in every scan mode and job size -----------------------------------------
@pytest.mark.usefixtures("numerics")
def test_adaptive_batch_equals_the_single_view_runs(case32):
    import torch
    ref, seg, smp = case32.single_adaptive([TOL])          # (once per numerics mode: the decisions may differ between the modes)
    for scan in SCANS:
        for jp in (0, 1, 4, 16):
            b = case32.views()
            try:
                d_img = torch.full((3 * W48 * H27 * 3,), -1.0, dtype=torch.float32, device="cuda:0")
                ok(batch_adapt(b, TOL, SCANS[scan], jp, d_out=d_img.data_ptr()), b[0])
                st = b[0].stats()
                torch.cuda.synchronize()
                out = frames(d_img, b)
                for v in range(3):
                    assert_same_state(state(b[v], True), ref[v], (scan, jp, v))
                    assert _same(out[v], ref[v]["resolve"]), (scan, jp, v)
                assert st.samples == sum(a.ainfo()["samples"] for a in b) == smp, (scan, jp)
                assert st.segments == seg, (scan, jp)
            finally:
                close(b)


# ---- 4. refinement, both ways ---------------------------------------------------------------------------------------------------------
def test_refinement_mixes_batched_and_single_calls(case32, singles32):
    fine = singles32[TOL_FINE][0]
    b, s = case32.views(), case32.views()
    try:
        ok(batch_adapt(b, TOL), b[0])                           # batch at 0.1, then single calls at 0.08
        for v in range(3):
            assert_same_state(state(b[v], True), singles32[TOL][0][v], v)
            b[v].run_ok(TOL_FINE)
        for a in s:                                             # single calls at 0.1, then the batch at 0.08
            a.run_ok(TOL)
        ok(batch_adapt(s, TOL_FINE), s[0])
        for v in range(3):
            for got in (state(b[v], True), state(s[v], True)):
                for k in ("words", "chunks", "info", "ranges", "resolve"):
                    assert _same(got[k], fine[v][k]) if isinstance(got[k], np.ndarray) else got[k] == fine[v][k], (v, k)
                assert {k: got["ainfo"][k] for k in got["ainfo"] if k != "rounds"} == {k: fine[v]["ainfo"][k] for k in fine[v]["ainfo"] if k != "rounds"}
        # the rounds of a refinement are the single refinement's: view by view, a batch refined by singles == singles refined by a batch
        r = case32.single_adaptive([TOL, TOL_FINE])[0]
        for v in range(3):
            assert b[v].ainfo()["rounds"] == s[v].ainfo()["rounds"] == r[v]["ainfo"]["rounds"], v
        # views in DIFFERENT states: view 1 already refined to 0.08 alone, the others at 0.1 -> a batch at 0.08 re-checks the settled view
        # (no pass holds a tile of it: rounds 0, as the single call at an unchanged tolerance reports) and refines the others
        m, ms = case32.views(), case32.views()
        try:
            ok(batch_adapt(m, TOL), m[0])
            m[1].run_ok(TOL_FINE)
            ok(batch_adapt(m, TOL_FINE), m[0])
            for a in ms:
                a.run_ok(TOL)
            ms[1].run_ok(TOL_FINE)
            for a in ms:
                a.run_ok(TOL_FINE)
            for v in range(3):
                assert_same_state(state(m[v], True), state(ms[v], True), ("mixed", v))
            assert m[1].ainfo()["rounds"] == 0 and m[0].ainfo()["rounds"] > 0
        finally:
            close(m, ms)
        # the same tolerance again: nothing to decide, no pass
        ok(batch_adapt(s, TOL_FINE), s[0])
        assert [a.ainfo()["rounds"] for a in s] == [0, 0, 0] and s[0].stats().samples == 0
        for v in range(3):
            assert np.array_equal(s[v].words(), fine[v]["words"])
    finally:
        close(b, s)


# ---- 5. the extremes ------------------------------------------------------------------------------------------------------------------
def test_unreachable_and_loose_tolerances(case32):
    b = case32.views()
    try:                                                        # fresh at 1e-300: every listed pass holds all N * n_tiles tiles
        ok(batch_adapt(b, UNREACHABLE), b[0])
        assert b[0].stats().samples == 3 * W48 * H27 * SPP
        for v in range(3):
            assert (b[v].chunks() == SPP).all() and b[v].ainfo()["rounds"] == 4 and b[v].info()["complete"] == 1 and b[v].ranges() == [(0, SPP)]
            assert _same(b[v].resolve(), single(case32.flat, case32.cams[v], case32.T, W48, H27, SPP, DEPTH, SEEDS[v], n_chunks=SPP)), v
    finally:
        close(b)
    b = case32.views()
    try:
        ok(batch_adapt(b, TOL_LOOSE), b[0])
        for v in range(3):
            assert (b[v].chunks() == 16).all() and b[v].ainfo()["rounds"] == 1 and b[v].ranges() == [(0, 16)]
        assert b[0].stats().samples == 3 * W48 * H27 * 16
        ok(batch_adapt(b, UNREACHABLE), b[0])
        for v in range(3):
            assert (b[v].chunks() == SPP).all() and b[v].ainfo()["rounds"] == 3 and b[v].info()["complete"] == 1
            assert _same(b[v].resolve(), single(case32.flat, case32.cams[v], case32.T, W48, H27, SPP, DEPTH, SEEDS[v], n_chunks=SPP)), v
    finally:
        close(b)


# ---- 6. Float64, chunks of three samples ----------------------------------------------------------------------------------------------
def test_float64_batch_and_its_refinement(case64):
    import torch
    for tols in ([0.15], [0.15, 0.1]):
        ref, seg, smp = case64.single_adaptive(tols)
        b = case64.views()
        try:
            d_img = torch.full((2 * 24 * 13 * 3,), -1.0, dtype=torch.float64, device="cuda:0")
            for tol in tols:
                ok(batch_adapt(b, tol, d_out=d_img.data_ptr(), gamma=0), b[0])
            st = b[0].stats()
            torch.cuda.synchronize()
            out = frames(d_img, b)
            for v in range(2):
                assert_same_state(state(b[v], True), ref[v], (tols, v))
                assert _same(out[v], b[v].resolve(gamma=0)), (tols, v)
            assert (st.segments, st.samples) == (seg, smp), tols
        finally:
            close(b)


# ---- 7. shapes ------------------------------------------------------------------------------------------------------------------------
def test_one_view_is_the_single_call(case32, singles32):
    b = case32.views([1])
    try:
        ok(batch_adapt(b, TOL), b[0])
        assert_same_state(state(b[0], True), singles32[TOL][0][1])
    finally:
        close(b)
    b, s = case32.views([2]), case32.views([2])
    try:
        ok(batch_accum(b, 3, 11), b[0])
        assert s[0].add(3, 11) == 0
        assert_same_state(state(b[0], False), state(s[0], False))
    finally:
        close(b, s)


def test_five_views_of_a_two_pixel_frame(case32):
    """2 x 1 pixels: one tile of two valid pixels per view, five tiles in the batch -- the list, the queues and the grid at their smallest.
    The views: the three cameras with their seeds, then cameras 0 and 1 again with seed + 100.  On the CPU oracle's samples the tiles'
    ratios D / M at 16 / 32 / 48 chunks are .068 .061 .031 | .147 .047 .036 | .154 .090 .044 | .056 .026 .067 | .111 .073 .121, so
    tolerance 0.08 gives C_t = 16, 32, 48, 16, 32 with the nearest ratio (.073) 9 % away."""
    which, seeds = [0, 1, 2, 0, 1], {0: 7, 1: 18, 2: 1234574}
    def mk():
        vs = []
        for k, v in enumerate(which):
            vs.append(Ad(case32.flat, case32.cams[v], case32.T, 2, 1, SPP, DEPTH, seeds[v] + 100 * (k // 3), n_chunks=SPP, min_chunks=16, check_chunks=16))
        return vs
    b, s = mk(), mk()
    try:
        tol = 0.08
        ok(batch_adapt(b, tol), b[0])
        got = b[0].stats().samples                             # (rtw_stats: the calling thread's LAST call)
        smp = 0
        for a in s:
            a.run_ok(tol)
            smp += a.stats().samples
        assert got == smp
        for v in range(5):
            assert_same_state(state(b[v], True), state(s[v], True), v)
        assert len({int(a.chunks()[0]) for a in s}) == 3, "the five tiles stop at three different checkpoints"
    finally:
        close(b, s)


def test_null_seeds_mean_the_params_seed_for_every_view(case32):
    b, s = case32.views(seeds=(5, 5, 5)), case32.views(seeds=(5, 5, 5))
    try:
        ok(batch_adapt(b, TOL, seeds=None), b[0])
        for v in range(3):
            s[v].run_ok(TOL)
            assert_same_state(state(b[v], True), state(s[v], True), v)
    finally:
        close(b, s)
    b, s = case32.views(seeds=(5, 5, 5)), case32.views(seeds=(5, 5, 5))
    try:
        ok(batch_accum(b, 0, 4, seeds=None), b[0])
        for v in range(3):
            assert s[v].add(0, 4) == 0
            assert_same_state(state(b[v], False), state(s[v], False), v)
    finally:
        close(b, s)


# ---- 8. refusals that need real accumulators: every accumulator of the array stays as it is ------------------------------------------
def test_refusals_leave_every_accumulator_untouched(case32):
    b = case32.views()
    fresh = case32.views()
    small = case32.views([0], width=40, height=27)
    try:
        err = b[0].L.rtw_last_error
        ok(batch_adapt(b, TOL), b[0])
        everyone = b + fresh + small
        before = [(a.words().copy(), a.info()) for a in everyone]

        def untouched():
            for a, (w, i) in zip(everyone, before):
                assert np.array_equal(a.words(), w) and a.info() == i
        # one accumulator twice
        assert batch_adapt([b[0], b[1], b[0]], TOL_FINE) == -2 and b"two views" in err()
        assert batch_accum([fresh[0], fresh[0]], 0, 4) == -2 and b"two views" in err()
        # an accumulator of another size
        assert batch_adapt([fresh[0], small[0]], TOL) == -4 and b"view 1" in err()
        assert batch_accum([fresh[0], small[0]], 0, 4) == -4 and b"view 1" in err()
        # a mix of unbound and bound accumulators
        assert batch_adapt([b[0], fresh[1], b[2]], TOL_FINE) == -4 and b"view 1" in err()
        assert batch_adapt([fresh[0], b[1]], TOL_FINE) == -4
        # a view bound to another camera (views 0 and 1 exchanged), and to another seed
        assert batch_adapt(b, TOL_FINE, cams=[b[1].cam, b[0].cam, b[2].cam]) == -4 and b"another render" in err() and b"view 0" in err()
        assert batch_adapt(b, TOL_FINE, cams=[b[0].cam, b[1].cam, b[1].cam]) == -4 and b"view 2" in err()
        assert batch_adapt(b, TOL_FINE, seeds=b[0].C.make_seeds([7, 18, 99], 3)) == -4 and b"view 2" in err()
        # other adaptive parameters, a looser tolerance than one view's last
        assert batch_adapt(b, TOL_FINE, floor=FLOOR * 2) == -4
        b[1].run_ok(TOL_FINE)
        before[1] = (b[1].words().copy(), b[1].info())
        assert batch_adapt(b, 0.09) == -4 and b"looser" in err() and b"view 1" in err()
        # a progressive batch on adaptive accumulators
        assert batch_accum(b, 0, 4) == -2 and b"adaptive" in err()
        assert batch_accum([fresh[0], b[1]], 60, 4) == -2 and b"view 1" in err()
        untouched()
        # ... and after all that the batch still refines
        ok(batch_adapt(b, TOL_FINE), b[0])
        assert all(a.info()["complete"] == 1 for a in b)
    finally:
        close(b, fresh, small)


# ---- 9. the Python layer --------------------------------------------------------------------------------------------------------------
def test_python_batch_renderers(rtw):
    T = np.float32
    scene = rtw.scene_random_spheres(elem_type=T)
    cams = [rtw.t_cam1(elem_type=T), rtw.t_cam2(elem_type=T)]
    kw = dict(depth=8, min_chunks=16, check_chunks=16)
    imgs, spp_maps, infos = rtw.render_adaptive_batch(scene, cams, 64, 48, tolerance=0.05, seeds=[3, 4], **kw)
    assert imgs.shape == (2, 36, 64, 3) and spp_maps.shape == (2, 36, 64) and spp_maps.dtype == np.int32
    for v in range(2):
        img, spp_map, info = rtw.render_adaptive(scene, cams[v], 64, 48, tolerance=0.05, seed=3 + v, **kw)
        assert _same(imgs[v], img) and np.array_equal(spp_maps[v], spp_map)
        assert {k: infos[v][k] for k in info} == info
    with rtw.AdaptiveBatchRenderer(scene, cams, 64, 48, seeds=[3, 4], device=0, **kw) as ar:
        ar.run(1e9)
        assert (ar.tile_chunks() == 16).all() and ar.tile_chunks().shape == (2, 5, 8)
        ar.run(0.05, group_cull=True)
        assert _same(ar.images(), imgs) and np.array_equal(ar.samples_per_pixel(), spp_maps)
        assert ar.stats()["samples"] == sum(i["samples"] for i in infos) - 2 * 64 * 36 * 16
    with rtw.ProgressiveBatchRenderer(scene, cams, 64, 8, depth=8, seeds=[3, 4], device=0) as pr:
        pr.add_range(4, 4)
        pr.add_range(0, 4, scan_valu=True)
        assert pr.ranges(0) == pr.ranges(1) == [(0, 8)] and pr.info(1)["complete"] == 1
        got = pr.images()
        for v in range(2):
            assert _same(got[v], rtw.render(scene, cams[v], 64, 8, depth=8, seed=3 + v))
            assert pr.read_pixels(v).shape == (36, 64, 8)
