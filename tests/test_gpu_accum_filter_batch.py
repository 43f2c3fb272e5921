"""Batched passes over accumulators on the GPU (include/rtw_hip.h rtw_accum_resolve_batch_*, rtw_accum_features_batch_*, rtw_accum_noise_batch_*,
rtw_guided_filter_batch_device_*, rtw_accum_filtered_batch_*).  The contract: view v of each call is, bit for bit, the single-view entry
point on accums[v], cams[v], seeds[v].  So every comparison here is the batch against the single-view calls on the same GPU (which
tests/test_gpu_accum_denoise.py pins to the witnesses), ON THE BITS; NaN pixels are compared as a set.  Tolerance of the comparisons: NONE.

The main frame is tests/test_gpu_accum_denoise.py's: cfg2's scene at 48 x 27 (6 x 4 tiles, a ragged last tile row), 64 chunks of one sample,
checkpoints 16 / 32 / 48, seen by three views: the golden camera, the camera with lens_radius + 0.125, the golden camera with another seed.
The adaptive tolerance is taken from the device's own checkpoint-16 ratios as adaptive48 takes it; at least one view must hold two or more
distinct C_t (asserted on the accumulators before a batch is judged).  The views are rendered once per precision by ONE batched adaptive
call and only read afterwards (every call under test only reads its accumulators; test 6 asserts that)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import accum_denoise_ref as AR
import denoise_ref as DR
import test_gpu_accum_batch as AB
from conftest import CamObj
from test_gpu_accum_denoise import (DEPTH, H27, SEED, SPP, W48, AcD, GuidedFrame, _assert_same, _cfg2, _dparams, _held_samples, _lib_layout, _ratios_at_16,
                                    _tt)
from test_gpu_adaptive import FLOOR, _same

pytestmark = pytest.mark.gpu

PRECISIONS = [np.float32, np.float64]


def _sfx(T):
    return "f64" if T is np.float64 else "f32"


class Views:
    """N AcD views of one frame and the batched entry points on them, straight on the C ABI (device 0)"""

    def __init__(self, views):
        self.vs, self.a = list(views), views[0]
        self.T, self.L, self.Cm = self.a.T, self.a.L, self.a.C
        self.n, self.W, self.H = len(self.vs), self.a.width, self.a.height

    def arrays(self, which=None, cams=None, seeds="own"):
        vs = self.vs if which is None else [self.vs[v] for v in which]
        return AB._arrays(vs, seeds, cams) + (len(vs),)

    def _buf(self, n):
        return self.a._buf(n)

    def _frames(self, d, n, ch):
        import torch
        torch.cuda.synchronize()
        flat = d.cpu().numpy()
        e = self.W * self.H * ch
        out = [flat[v * e:(v + 1) * e] for v in range(n)]
        return [x.reshape(self.W, self.H, ch).transpose(1, 0, 2) if ch > 1 else x.reshape(self.W, self.H).T for x in out]

    def features_rc(self, d_ptr, flags=0, which=None, cams=None, seeds="own"):
        cm, sd, accs, n = self.arrays(which, cams, seeds)
        P = self.a._params(flags, 0, 1)
        return getattr(self.L, "rtw_accum_features_batch_" + _sfx(self.T))(self.a.scene, cm, n, sd, C.byref(P), accs, C.c_void_p(d_ptr), None)

    def features(self, flags=0, which=None):
        """rtw_accum_features_batch_* -> ([raw [H, W, 8] per view], stats)"""
        n = self.n if which is None else len(which)
        d = self._buf(n * self.W * self.H * 8)
        self.Cm.check(self.features_rc(d.data_ptr(), flags, which))
        st = self.a.stats()
        return self._frames(d, n, 8), st

    def resolve_rc(self, d_ptr, gamma=1, which=None):
        _, _, accs, n = self.arrays(which)
        return getattr(self.L, "rtw_accum_resolve_batch_" + _sfx(self.T))(accs, n, gamma, C.c_void_p(d_ptr), None)

    def resolve(self, gamma=1, which=None):
        n = self.n if which is None else len(which)
        d = self._buf(n * self.W * self.H * 3)
        self.Cm.check(self.resolve_rc(d.data_ptr(), gamma, which))
        return self._frames(d, n, 3)

    def noise_rc(self, d_ptr, which=None):
        _, _, accs, n = self.arrays(which)
        return getattr(self.L, "rtw_accum_noise_batch_" + _sfx(self.T))(accs, n, C.c_void_p(d_ptr), None)

    def noise(self, which=None):
        n = self.n if which is None else len(which)
        d = self._buf(n * self.W * self.H)
        self.Cm.check(self.noise_rc(d.data_ptr(), which))
        return self._frames(d, n, 1)

    def filtered_rc(self, out, guided, gamma=1, which=None, cams=None, seeds="own", **kw):
        cm, sd, accs, n = self.arrays(which, cams, seeds)
        P = self.a._params(0, 0, gamma)
        D = _dparams(gamma=1 - gamma, **kw)                    # (d->gamma is replaced by p->gamma: hand in the opposite)
        fn = getattr(self.L, "rtw_accum_filtered_batch_" + _sfx(self.T))
        return fn(self.a.scene, cm, n, sd, C.byref(P), C.byref(D), accs, guided, out.ctypes.data_as(C.c_void_p))

    def filtered(self, guided, gamma=1, which=None, **kw):
        n = self.n if which is None else len(which)
        out = np.full(n * self.W * self.H * 3, -7.0, self.T)
        self.Cm.check(self.filtered_rc(out, guided, gamma, which, **kw))
        e = self.W * self.H * 3
        return [out[v * e:(v + 1) * e].reshape(self.W, self.H, 3).transpose(1, 0, 2) for v in range(n)]

    def close(self):
        AB.close(self.vs)


def _cams3():
    flat, cam = _cfg2()
    cam2 = CamObj(dict(cam.__dict__, lens_radius=np.asarray(cam.lens_radius) + np.asarray(cam.lens_radius).dtype.type(0.125)))
    return flat, [cam, cam2, cam], [SEED, SEED, SEED + 5]


def _views48(T, **kw):
    flat, cams, seeds = _cams3()
    return [AcD(flat, cm, T, W48, H27, SPP, DEPTH, sd, n_chunks=SPP, min_chunks=16, check_chunks=16, **kw) for cm, sd in zip(cams, seeds)]


def _adaptive_views48(T):
    """three adaptive views after ONE batched adaptive call; the tolerance is the middle of a gap of view 0's checkpoint-16 ratios"""
    r = np.sort(_ratios_at_16(T))
    for rank in (7, 5, 9, 11):
        tol = 0.5 * (r[rank - 1] + r[rank])
        vs = _views48(T)
        AB.ok(AB.batch_adapt(vs, tol), vs[0])
        if any(len(set(int(c) for c in a.chunks())) >= 2 for a in vs):
            return Views(vs), tol
        AB.close(vs)
    pytest.fail(f"no candidate tolerance left a view with two distinct C_t: ratios {r}")


_shared = {}


@pytest.fixture(scope="module")
def adaptive3():
    """T -> (Views, tolerance, the per-view references of the single calls): made once per precision, only read afterwards"""
    def get(T):
        if T not in _shared:
            V, tol = _adaptive_views48(T)
            ref = dict(feat={}, resolve={g: [np.ascontiguousarray(a.resolve(g)) for a in V.vs] for g in (0, 1)}, noise=[np.ascontiguousarray(a.noise()) for a in V.vs])
            _shared[T] = (V, tol, ref)
        return _shared[T]
    yield get
    for V, _, _ in _shared.values():
        V.close()
    _shared.clear()


# ---- 1. batched tiled features ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 4])
@pytest.mark.parametrize("T", PRECISIONS)
def test_batched_tiled_features_equal_the_single_calls(adaptive3, T, flags):
    V, tol, ref = adaptive3(T)
    assert any(len(set(int(c) for c in a.chunks())) >= 2 for a in V.vs), [a.chunks() for a in V.vs]      # the reference alone meets the census
    singles = [np.ascontiguousarray(a.features(flags)[0]) for a in V.vs]
    raws, st = V.features(flags)
    for v in range(V.n):
        _assert_same(raws[v], singles[v], f"{np.dtype(T).name} flags {flags}: view {v} of 3")
        assert not (raws[v] == -7.0).all(axis=2).any()                # every pixel was written
    held = [_held_samples(a) for a in V.vs]
    assert st.samples == st.segments == sum(held) and st.sphere_tests == st.segments * V.a.flat["n"] and st.kernel_ms > 0
    for v in (0, 2):                                                  # n_views = 1: a batch of one runs the batched instance
        one, st1 = V.features(flags, which=[v])
        _assert_same(one[0], singles[v], f"a batch of view {v} alone")
        assert st1.samples == st1.segments == held[v]


# ---- 2. frames of one tile: the waves of a workgroup belong to different views with different trip counts ------------------------------------
def _one_tile_views(T, W, H, n_views):
    """n_views views of a W x H frame of ONE tile, 32 chunks of one sample, checkpoints 8 / 16 / 24, seeds 21 ..; the tolerance is the middle of
    the widest gap between the views' checkpoint-8 ratios (measured on the device, every tile stopped at 8), so C_t takes >= 2 values"""
    from rtw_amd import reference_decisions
    flat, cam = _cfg2()
    mk = lambda: [AcD(flat, cam, T, W, H, 32, DEPTH, 21 + v, n_chunks=32, min_chunks=8, check_chunks=8) for v in range(n_views)]
    vs = mk()
    try:
        AB.ok(AB.batch_adapt(vs, 1e30), vs[0])
        ratios = []
        for a in vs:
            assert (a.chunks() == 8).all()
            _, D, _, M = reference_decisions(a.words(), W, H, 8, 1.0, FLOOR, return_terms=True)
            ratios.append(D[0] / M[0])
    finally:
        AB.close(vs)
    r = np.sort(ratios)
    k = int(np.argmax(r[1:] - r[:-1]))
    assert r[k + 1] > r[k], r
    vs = mk()
    AB.ok(AB.batch_adapt(vs, 0.5 * (r[k] + r[k + 1])), vs[0])
    return Views(vs)


@pytest.mark.parametrize("W,H,n_views", [(8, 8, 6), (1, 1, 5)])
@pytest.mark.parametrize("T", PRECISIONS)
def test_frames_of_one_tile(T, W, H, n_views):
    V = _one_tile_views(T, W, H, n_views)
    try:
        ct = [int(a.chunks()[0]) for a in V.vs]
        assert len(set(ct)) >= 2, ct                                  # the waves of the first workgroup run different trip counts
        for flags in (0, 4):
            raws, st = V.features(flags)
            for v, a in enumerate(V.vs):
                _assert_same(raws[v], np.ascontiguousarray(a.features(flags)[0]), f"{W}x{H} flags {flags}: view {v}, C_t {ct[v]}")
            assert st.samples == W * H * sum(ct)
        for g in (0, 1):
            for v, (x, a) in enumerate(zip(V.resolve(g), V.vs)):
                _assert_same(x, np.ascontiguousarray(a.resolve(g)), f"{W}x{H} resolve gamma {g}: view {v}")
        for v, (x, a) in enumerate(zip(V.noise(), V.vs)):
            _assert_same(x, np.ascontiguousarray(a.noise()), f"{W}x{H} noise: view {v}")
        for v, (x, a) in enumerate(zip(V.filtered(1), V.vs)):
            _assert_same(x, np.ascontiguousarray(a.filtered(1)), f"{W}x{H} the one call: view {v}")
    finally:
        V.close()


# ---- 3. uniform accumulators; the refusals that look into an accumulator -------------------------------------------------------------------------
@pytest.mark.parametrize("T", PRECISIONS)
def test_uniform_accumulators_and_the_refusals(adaptive3, T):
    import torch
    V = Views(_views48(T))
    A, _, _ = adaptive3(T)
    err = V.L.rtw_last_error
    try:
        d = V._buf(3 * W48 * H27 * 8)
        out = np.zeros(3 * W48 * H27 * 3, T)
        assert V.features_rc(d.data_ptr()) == -2 and b"no chunk interval" in err()                     # nothing held
        assert V.resolve_rc(d.data_ptr()) == -2 and b"no samples" in err()
        AB.ok(AB.batch_accum(V.vs, 8, 16), V.a)
        raws, st = V.features()
        for v, a in enumerate(V.vs):
            _assert_same(raws[v], np.ascontiguousarray(a.features()[0]), f"uniform [8, 24): view {v}")
        assert st.samples == 3 * W48 * H27 * 16
        for g in (0, 1):
            for v, (x, a) in enumerate(zip(V.resolve(g), V.vs)):
                _assert_same(x, np.ascontiguousarray(a.resolve(g)), f"uniform resolve gamma {g}: view {v}")
        for v, (x, a) in enumerate(zip(V.filtered(0, sigma_color=0.5), V.vs)):
            _assert_same(x, np.ascontiguousarray(a.filtered(0, sigma_color=0.5)), f"uniform, the plain one call: view {v}")
        assert V.filtered_rc(out, 1) == -2 and b"not adaptive" in err()                                # guided needs word 7
        assert V.noise_rc(d.data_ptr()) == -2 and b"not adaptive" in err()
        # a mix of the two kinds: the resolve takes it, the feature pass does not
        mixed = Views([V.vs[0], A.vs[1], V.vs[2]])
        assert mixed.features_rc(d.data_ptr()) == -2 and b"all adaptive or all uniform" in err()
        assert mixed.filtered_rc(out, 0) == -2
        for v, (x, a) in enumerate(zip(mixed.resolve(0), mixed.vs)):
            _assert_same(x, np.ascontiguousarray(a.resolve(0)), f"a mixed resolve: view {v}")
        # not the binding: view 1 with view 0's camera -> -4; a batch in another order with its own cameras is fine
        flat, cams, seeds = _cams3()
        assert V.features_rc(d.data_ptr(), cams=[cams[0], cams[0], cams[2]]) == -4 and b"view 1" in err() and b"another render" in err()
        assert V.features_rc(d.data_ptr(), seeds=V.Cm.make_seeds([SEED, SEED, SEED], 3)) == -4 and b"view 2" in err()
        assert V.filtered_rc(out, 0, seeds=V.Cm.make_seeds([SEED, SEED, SEED], 3)) == -4
        assert V.features_rc(d.data_ptr(), which=[2, 0]) == 0
        assert V.features_rc(d.data_ptr(), flags=5) == 0                                               # scan flags may differ from the passes'
        # another size, another precision -> -4
        other = AcD(flat, cams[0], T, 8, 5, SPP, DEPTH, SEED, n_chunks=SPP)
        wrong = AcD(flat, cams[0], np.float32 if T is np.float64 else np.float64, W48, H27, SPP, DEPTH, SEED, n_chunks=SPP)
        try:
            assert other.add(8, 16) == 0 and wrong.add(8, 16) == 0
            assert Views([V.vs[0], other]).resolve_rc(d.data_ptr()) == -4 and b"view 1" in err()
            assert Views([V.vs[0], other]).features_rc(d.data_ptr()) == -4
            assert Views([V.vs[0], wrong]).resolve_rc(d.data_ptr()) == -4 and b"precision" in err()
        finally:
            other.close()
            wrong.close()
        # differing intervals -> -2
        assert V.vs[1].add(24, 4) == 0
        assert V.features_rc(d.data_ptr()) == -2 and b"ONE interval" in err()
        assert V.filtered_rc(out, 0) == -2
        assert V.vs[0].add(40, 2) == 0                                                                 # a second interval in view 0
        assert V.features_rc(d.data_ptr()) == -2 and b"2 chunk intervals" in err()
        for v, (x, a) in enumerate(zip(V.resolve(1), V.vs)):                                           # the resolve takes any ranges: per-view divisors
            _assert_same(x, np.ascontiguousarray(a.resolve(1)), f"resolve of views with different ranges: view {v}")
        torch.cuda.synchronize()
    finally:
        V.close()


# ---- 4. batched resolve and noise map ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", PRECISIONS)
def test_batched_resolve_and_noise_map_equal_the_single_calls_and_the_witness(adaptive3, T):
    V, tol, ref = adaptive3(T)
    for g in (0, 1):
        got = V.resolve(g)
        for v in range(V.n):
            _assert_same(got[v], ref["resolve"][g][v], f"adaptive resolve gamma {g}: view {v}")
    got = V.noise()
    for v, a in enumerate(V.vs):
        _assert_same(got[v], ref["noise"][v], f"noise map: view {v}")
        wit = AR.noise_map(a.words(), a.chunks(), W48, H27, SPP, 1, FLOOR, T)
        assert np.isfinite(wit).all() and (wit > 0).any()
        _assert_same(got[v], wit, f"noise map against the witness: view {v}")
    one = V.noise(which=[1])
    _assert_same(one[0], ref["noise"][1], "a batch of view 1 alone")
    # accumulators with another dark_floor than view 0's -> -4 (the kernel takes one set)
    flat, cams, seeds = _cams3()
    b = AcD(flat, cams[0], T, W48, H27, SPP, DEPTH, SEED + 9, n_chunks=SPP, min_chunks=16, check_chunks=16, floor=2 * FLOOR)
    try:
        b.run_ok(1e30)
        d = V._buf(2 * W48 * H27)
        assert Views([V.vs[0], b]).noise_rc(d.data_ptr()) == -4 and b"dark_floor" in V.L.rtw_last_error()
        assert Views([V.vs[0], V.vs[0]]).noise_rc(d.data_ptr()) == -2 and b"two views" in V.L.rtw_last_error()
        for v, (x, a) in enumerate(zip(Views([V.vs[0], b]).resolve(1), (V.vs[0], b))):                 # the resolve does not care
            _assert_same(x, np.ascontiguousarray(a.resolve(1)), f"resolve beside another dark_floor: view {v}")
    finally:
        b.close()


# ---- 5. the guided batched filter on hand-made frames -------------------------------------------------------------------------------------------------
class GuidedBatch:
    """N hand-made frames of one size (DR.handmade / AR.special_noise with N seeds) one behind the other on the device"""

    def __init__(self, W, H, T, seeds):
        import torch
        from rtw_amd import _capi
        self.L, self.T, self.W, self.H, self.n = _capi.lib(), T, W, H, len(seeds)
        self.frames = [(DR.handmade(H, W, T, s), AR.special_noise(H, W, T, s + 100)) for s in seeds]
        cat = lambda xs: torch.from_numpy(np.concatenate([_lib_layout(x).reshape(-1) for x in xs])).to("cuda:0")
        self.img, self.feat = cat([f[0][0] for f in self.frames]), cat([f[0][1] for f in self.frames])
        self.noise = cat([f[1] for f in self.frames])
        self.work_elems = self.n * int(self.L.rtw_denoise_work_bytes(W, H, np.dtype(T).itemsize)) // np.dtype(T).itemsize
        torch.cuda.synchronize()

    def run(self, noise=None, poison=False, **kw):
        import torch
        from rtw_amd import _capi
        work = torch.full((self.work_elems,), float("nan") if poison else 0.0, dtype=_tt(self.T), device="cuda:0")
        out = torch.full((self.n * self.W * self.H * 3,), -7.0, dtype=_tt(self.T), device="cuda:0")
        noise = self.noise if noise is None else noise
        torch.cuda.synchronize()
        D = _dparams(**kw)
        fn = getattr(self.L, "rtw_guided_filter_batch_device_" + _sfx(self.T))
        _capi.check(fn(C.byref(D), self.W, self.H, self.n, C.c_void_p(self.img.data_ptr()), C.c_void_p(self.feat.data_ptr()), C.c_void_p(noise.data_ptr()),
                       C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr()), None))
        torch.cuda.synchronize()
        e = self.W * self.H * 3
        flat = out.cpu().numpy()
        return [flat[v * e:(v + 1) * e].reshape(self.W, self.H, 3).transpose(1, 0, 2) for v in range(self.n)]


@pytest.mark.parametrize("W,H", [(1, 1), (5, 3), (37, 23)])
@pytest.mark.parametrize("T", PRECISIONS)
def test_guided_batched_frames_equal_the_witness_view_by_view(T, W, H):
    B = GuidedBatch(W, H, T, (31, 32, 33))
    for levels in (1, 3, 5):
        for demodulate in (True, False):
            for gamma in (0, 1):
                kw = dict(levels=levels, demodulate=demodulate, gamma=gamma)
                got = B.run(**kw)
                for v, ((image, feat), noise) in enumerate(B.frames):
                    _assert_same(got[v], AR.guided(image, feat, noise, T, **kw), f"{np.dtype(T).name} {W}x{H} {kw}: view {v}")
    # the middle view's noise all NaN: it is all NaN, the outer views are unchanged -- no tap crosses a view
    base = B.run(levels=5)
    noise = B.noise.clone()
    noise[W * H:2 * W * H] = float("nan")
    got = B.run(noise=noise, levels=5)
    assert np.isnan(got[1]).all()
    _assert_same(got[0], base[0], "view 0 beside a view without a valid pixel")
    _assert_same(got[2], base[2], "view 2 beside a view without a valid pixel")
    # a workspace full of NaN
    for v, x in enumerate(B.run(poison=True, levels=5)):
        _assert_same(x, base[v], f"a workspace full of NaN: view {v}")


@pytest.mark.parametrize("T", PRECISIONS)
def test_the_guided_batch_of_one_equals_the_single_frame_entry_point(T):
    """the same frame through rtw_guided_filter_device_* (GuidedFrame) and as a batch of three copies"""
    import torch
    W, H = 37, 23
    one = GuidedFrame(W, H, T)
    ref = one.image(one.run(levels=3))
    B = GuidedBatch(W, H, T, (31,))
    B.n, B.img, B.feat, B.noise = 3, one.img.reshape(-1).repeat(3), one.feat.reshape(-1).repeat(3), one.noise.reshape(-1).repeat(3)
    B.work_elems *= 3
    torch.cuda.synchronize()
    for v, x in enumerate(B.run(levels=3)):
        _assert_same(x, ref, f"copy {v}")


# ---- 6. the one call --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_one_call_equals_the_single_calls_and_leaves_the_accumulators_alone(T):
    V, tol = _adaptive_views48(T)                                      # (its own views: the test refines them)
    try:
        before = [(a.words().copy(), a.chunks().copy(), a.ainfo()) for a in V.vs]
        for guided, kw in ((1, {}), (0, dict(sigma_color=0.5)), (1, dict(levels=2, demodulate=False, sigma_color=2.0))):
            for gamma in (0, 1):
                got = V.filtered(guided, gamma, **kw)
                st = V.a.stats()                                       # the ONE feature launch's record
                assert st.samples == st.segments == sum(_held_samples(a) for a in V.vs)
                for v, a in enumerate(V.vs):
                    _assert_same(got[v], np.ascontiguousarray(a.filtered(guided, gamma, **kw)), f"guided {guided} gamma {gamma} {kw}: view {v}")
        _assert_same(V.filtered(1, which=[2])[0], np.ascontiguousarray(V.vs[2].filtered(1)), "a batch of view 2 alone")
        for a, (w, ct, info) in zip(V.vs, before):
            assert _same(a.words(), w) and np.array_equal(a.chunks(), ct) and a.ainfo() == info
        # a refinement afterwards equals a fresh run at the smaller tolerance
        AB.ok(AB.batch_adapt(V.vs, 0.5 * tol), V.a)
        fresh = _views48(T)
        try:
            AB.ok(AB.batch_adapt(fresh, 0.5 * tol), fresh[0])
            for v, (a, b) in enumerate(zip(V.vs, fresh)):
                assert _same(a.words(), b.words()) and np.array_equal(a.chunks(), b.chunks()), v
            for v, (x, y) in enumerate(zip(V.filtered(1), Views(fresh).filtered(1))):
                _assert_same(x, y, f"the one call after a refinement: view {v}")
        finally:
            AB.close(fresh)
    finally:
        V.close()


# ---- 7. the instance the batched feature call runs -------------------------------------------------------------------------------------------------
_PROBE = """
import sys
sys.path[:0] = [{tests!r}, {root!r}, {oracle!r}]
import torch
torch.cuda.init()                       # (two HIP runtimes in one process: torch's goes first, tests/conftest.py)
import numpy as np
import big_scenes as BS
import test_gpu_accum_batch as AB
import test_gpu_accum_denoise as G
import test_gpu_accum_filter_batch as FB
from rtw_amd import reference_decisions
T = np.float32
big = sys.argv[1] == "big"
flat = BS.scene(T) if big else G._cfg2()[0]
cams = BS.cameras(T)[:2] if big else FB._cams3()[1][:2]
mk = lambda: [G.AcD(flat, cm, T, 48, 27, 32, 8, 7 + v, n_chunks=32, min_chunks=8, check_chunks=8) for v, cm in enumerate(cams)]
vs = mk()
AB.ok(AB.batch_adapt(vs, 1e30), vs[0])
_, D, _, M = reference_decisions(vs[0].words(), 48, 27, 8, 1.0, G.FLOOR, return_terms=True)
r = np.sort([d / m for d, m in zip(D, M)])
AB.close(vs)
vs = mk()
AB.ok(AB.batch_adapt(vs, 0.5 * (r[11] + r[12])), vs[0])
V = FB.Views(vs)
print("@features", file=sys.stderr, flush=True)
raws, st = V.features()
print("@end", file=sys.stderr, flush=True)
for v, a in enumerate(vs):
    G._assert_same(raws[v], np.ascontiguousarray(a.features()[0]), "view %d" % v)
assert st.samples == sum(G._held_samples(a) for a in vs)
print("distinct", max(len(set(int(c) for c in a.chunks())) for a in vs))
V.close()
"""
_LINE = re.compile(r"\[rtw debug\] features instance: (f32|f64) lds_scene=(\d) cull=(\d) mfma=(\d) fixed=(\d) batch=(\d) accum=(\d) adapt=(\d) lds_bytes=(\d+) "
                   r"blocks_per_cu=(\d+)( views=(\d+))?\s*$", re.M)


@pytest.mark.parametrize("which,lds_scene", [("lds", 1), ("big", 0)])
def test_the_tiled_batched_instance(which, lds_scene):
    """a fresh process, because the RTW_DEBUG aid is read once per process: between the marks around ONE batched feature call over adaptive
    accumulators there is exactly one `features instance` line, and it names the TILED && BATCH instance -- for cfg2's scene (staged in LDS)
    and for tests/big_scenes.py's 1600-sphere scene (read from global memory)"""
    import big_scenes as BS
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    code = _PROBE.format(tests=tests, root=root, oracle=os.path.join(root, "oracle"))
    env = dict(os.environ, RTW_ENABLE_TEST_AIDS="1", RTW_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", code, which], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert int(r.stdout.split("distinct")[1].split()[0]) >= 2, r.stdout
    section = r.stderr.split("@features")[1].split("@end")[0]
    lines = _LINE.findall(section)
    assert len(lines) == 1, section[-500:]
    prec, lds, cull, mfma, fixed, batch, accum, adapt, _, _, _, n = lines[0]
    assert (prec, int(lds), int(cull), int(mfma), int(batch), int(accum), int(adapt), n) == ("f32", lds_scene, 0, 1, 1, 1, 1, "2"), lines[0]
    # the single-view tiled passes behind the mark keep their text: the existing parser reads them, and they say batch=0
    rest = BS.parse_instance_lines(r.stderr.split("@end")[1])
    assert len(rest) == 2 and all(i.kernel == "features" and (i.accum, i.adapt, i.batch) == (1, 1, 0) for i, _, _ in rest), rest


# ---- 8. the Python layer ---------------------------------------------------------------------------------------------------------------------------
def test_the_python_layer(rtw):
    """the package's own random-spheres scene at 64 x 36, 48 chunks of one sample, checkpoints 16 / 32, two views"""
    T, W, S = np.float32, 64, 48
    scene = rtw.scene_random_spheres(elem_type=T)
    cams, seeds = [rtw.t_cam1(elem_type=T), rtw.t_default_cam(elem_type=T)], [3, 11]
    kw = dict(dark_floor=FLOOR, min_chunks=16, check_chunks=16, depth=DEPTH)
    with rtw.AdaptiveBatchRenderer(scene, cams, W, S, seeds=seeds, **kw) as ab:
        ab.run(0.05)
        assert len(set(int(c) for c in ab.tile_chunks().reshape(-1))) >= 2
        den = ab.denoised_all()
        assert den.shape == (2, 36, 64, 3) and den.dtype == T
        for v in range(2):
            _assert_same(den[v], ab.denoised(v), f"AdaptiveBatchRenderer.denoised_all: view {v}")
        plain = ab.denoised_all(guided=False, gamma=False, levels=2)
        noise, feat, imgs = ab.noise_all(), ab.features_all(), ab.images(gamma=False)
        assert noise.shape == (2, 36, 64) and feat["raw"].shape == (2, 36, 64, 8) and feat["coverage"].shape == (2, 36, 64)
        for v in range(2):
            _assert_same(plain[v], ab.denoised(v, guided=False, gamma=False, levels=2), f"denoised_all(guided=False): view {v}")
            with rtw.AdaptiveRenderer(scene, cams[v], W, S, seed=seeds[v], **kw) as one:
                one.run(0.05)
                _assert_same(noise[v], one.noise(), f"noise_all: view {v}")
                _assert_same(imgs[v], one.image(gamma=False), f"images() through the batched resolve: view {v}")
                _assert_same(np.ascontiguousarray(feat["raw"][v]), np.ascontiguousarray(one.features()["raw"]), f"features_all: view {v}")
        import torch
        buf = ab._device_buffer(2 * 36 * 64 * 3)
        ab.images_into(buf.data_ptr(), gamma=True, stream=torch.cuda.current_stream(buf.device).cuda_stream)
        into = buf.cpu().numpy().reshape(2, 64, 36, 3).transpose(0, 2, 1, 3)
        _assert_same(into, ab.images(), "images_into against images()")
    imgs, spp_map, infos = rtw.render_adaptive_denoised_batch(scene, cams, W, S, tolerance=0.05, seeds=seeds, **kw)
    _assert_same(imgs, den, "render_adaptive_denoised_batch")
    assert spp_map.shape == (2, 36, 64) and len(infos) == 2 and infos[0]["n_tiles"] == 40
    with rtw.ProgressiveBatchRenderer(scene, cams, W, S, depth=DEPTH, seeds=seeds) as pb:
        pb.add_range(3, 8)
        den = pb.denoised_all(gamma=False)
        feat, imgs = pb.features_all(), pb.images()
        for v in range(2):
            with rtw.ProgressiveRenderer(scene, cams[v], W, S, depth=DEPTH, seed=seeds[v]) as one:
                one.add_range(3, 8)
                _assert_same(imgs[v], one.image(), f"ProgressiveBatchRenderer.images: view {v}")
            _assert_same(den[v], pb.denoised(v, gamma=False), f"ProgressiveBatchRenderer.denoised_all: view {v}")
            ref = rtw.render_features(scene, cams[v], W, S, seed=seeds[v], chunks=(3, 8))["raw"]
            _assert_same(np.ascontiguousarray(feat["raw"][v]), np.ascontiguousarray(ref), f"ProgressiveBatchRenderer.features_all: view {v}")


# ---- 4b. the batched resolve on hand-made words: a divisor per view, every class of sum, poisoned pixels ---------------------------------------
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_batched_resolve_on_hand_made_words(T):
    """tests/test_gpu_accum_words.py's imported accumulators (rtw_accum_import takes any words): the frames of accum_words.resolve_classes --
    every shift count of the normalisation, ties, carries, 2^127 - 1 and -2^127 --, each view with ITS OWN divisor (1, 3, 1000, 2^31 - 1 and
    the two intervals that hold 6 samples), a poisoned pixel with INT64_MIN in word 7 per view; then five frames of 1 x 1.  Against the exact
    witness accum_words.resolve, per view."""
    import torch
    import accum_words as AW
    import test_gpu_accum_words as GW
    from rtw_amd import _capi
    L = _capi.lib()
    fn = getattr(L, "rtw_accum_resolve_batch_" + _sfx(T))
    divisors = [1, 3, 1000, 2 ** 31 - 1, 6]
    frames = GW.class_frames()
    big = []
    for k, dv in enumerate(divisors):
        w = frames[k % len(frames)].copy()
        AW.set_pixel(w, k, 10 - k, rgb=(AW.fx(0.5), AW.fx(0.25), AW.fx(2)), h=-2 ** 63, poison=k + 1)
        big.append((w, dv, GW.W, GW.H))
    tiny = [(AW.words_of_sums([AW.fx(k + 0.5), -AW.fx(0.125), AW.fx(3)], 1, 1), dv, 1, 1) for k, dv in enumerate(divisors)]
    for group in (big, tiny):
        width, height = group[0][2], group[0][3]
        accs = [GW.Imported(GW._blob(w, T, dv, width, height)) for w, dv, _, _ in group]
        try:
            handles = _capi.make_handles([a.acc for a in accs])
            e = width * height * 3
            for gamma in (0, 1):
                d = torch.full((len(accs) * e,), -7.0, dtype=_tt(T), device="cuda:0")
                torch.cuda.synchronize()
                _capi.check(fn(handles, len(accs), gamma, C.c_void_p(d.data_ptr()), None))
                torch.cuda.synchronize()
                flat = d.cpu().numpy()
                for v, (w, dv, _, _) in enumerate(group):
                    got = AW.from_device_order(flat[v * e:(v + 1) * e], width, height, 3)
                    ref = AW.resolve(w, dv, gamma, T)
                    assert AW.same_bits(got, ref), (width, height, v, dv, gamma)
                    assert AW.same_bits(accs[v].resolve_device(gamma, T), ref)          # ... which is also the single kernel's
            if width > 1:
                assert all(np.isnan(AW.from_device_order(flat[v * e:(v + 1) * e], width, height, 3)[v, 10 - v]).all() for v in range(len(accs)))
        finally:
            for a in accs:
                a.close()


# ---- 4c. unit ops 30 / 31: the batched resolve and the batched noise map on hand-made words and made-up C_t ----------------------------------------
def unit_read_batch(op, views, width, height, spp, cs, slot4, T):
    """rtw_unit_* op 30 (slot4 = gamma) / 31 (slot4 = dark_floor) on `views` = [(C_t, words H x W x 8)] -> (the single kernel's frames view by
    view, the frames of ONE launch of the batch kernel), each a list of H x W x 3 (30) / H x W (31) arrays of type T"""
    import accum_words as AW
    from rtw_amd import _capi
    L = _capi.lib()
    ch = 3 if op == 30 else 1
    x = [np.array([width, height, spp, cs, slot4, 0, 0, 0], np.float64).view(np.uint64)]
    for chunks, words in views:
        x += [np.array(chunks, np.float64).view(np.uint64), AW.device_order(words, 8)]
    x = np.concatenate(x)
    per = width * height * ch
    y = np.full(2 * len(views) * per, -9.0, np.float64)
    fn = L.rtw_unit_f64 if T is np.float64 else L.rtw_unit_f32
    _capi.check(fn(op, len(views), x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), None, None))
    back = y.astype(T)
    assert AW.same_bits(back.astype(np.float64), y)                   # (every slot holds a value of type T)
    frame = lambda k: AW.from_device_order(back[k * per:(k + 1) * per], width, height, ch) if ch == 3 else back[k * per:(k + 1) * per].reshape(width, height).T
    n = len(views)
    return [frame(v) for v in range(n)], [frame(n + v) for v in range(n)]


def _random_views(width, height, n_views, seed, max_chunks):
    import accum_words as AW
    rng = np.random.default_rng(seed)
    n_tiles = ((height + 7) // 8) * ((width + 7) // 8)
    return [(rng.integers(1, max_chunks + 1, size=n_tiles), AW.random_words(width, height, seed + 10 * v)) for v in range(n_views)]


@pytest.mark.parametrize("T", PRECISIONS)
def test_the_batched_noise_kernel_on_hand_made_words(T):
    """accum_denoise_ref.noise_cases (a poisoned centre and neighbour, INT64_MIN in word 7, neighbouring tiles with different C_t, the ragged
    last tile row) as views of ONE launch next to views of random words and other C_t; then frames of 1 x 1, 5 x 3 and 9 x 17 with made-up
    C_t per view.  Against accum_denoise_ref.noise_map per view; the single-kernel half and the batch half are identical."""
    import accum_words as AW
    for name, words, floor, expect in AR.noise_cases():
        views = [(AR.NCHUNKS, words), (AR.NCHUNKS[::-1], AW.random_words(AR.NW, AR.NH, 3)), ([1, 1, 7, 2], words)]
        single, batch = unit_read_batch(31, views, AR.NW, AR.NH, AR.NSPP, AR.NCS, floor, T)
        for v, (chunks, w) in enumerate(views):
            _assert_same(batch[v], AR.noise_map(w, chunks, AR.NW, AR.NH, AR.NSPP, AR.NCS, floor, T), f"{name}: view {v}")
            _assert_same(batch[v], single[v], f"{name}: view {v}, batch half against single half")
        for (i, j), want in expect.items():                            # ... and the expectations spelled out by hand, on view 0
            assert np.isnan(batch[0][i, j]) if want is None else batch[0][i, j] == np.dtype(T).type(want), (name, i, j)
    for width, height, n_views in ((1, 1, 5), (5, 3, 3), (9, 17, 3)):
        views = _random_views(width, height, n_views, 40 + width, 8)
        single, batch = unit_read_batch(31, views, width, height, 20, 3, 0.03, T)
        for v, (chunks, w) in enumerate(views):
            _assert_same(batch[v], AR.noise_map(w, chunks, width, height, 20, 3, 0.03, T), f"{width}x{height}: view {v}")
            _assert_same(batch[v], single[v], f"{width}x{height}: view {v}, batch half against single half")


@pytest.mark.parametrize("gamma", [0, 1])
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_batched_per_tile_resolve_on_hand_made_words(T, gamma):
    """the adaptive branch of the batched resolve (a divisor per tile, C_t per view): tests/test_gpu_accum_kernels.py's frames of every class
    of sum (ties, carries, 2^127 - 1, -2^127, poisoned pixels) with INT64_MIN in word 7 of a pixel, a different C_t array per view; then frames
    of 1 x 1, 5 x 3 and 9 x 17 of random words.  Against the exact witness accum_words.resolve over accum_words.tile_divisors per view; the
    single-kernel half and the batch half are identical."""
    import accum_words as AW
    import test_gpu_accum_kernels as GK
    spp, cs = 1000, 7
    frames = [f.copy() for f in GK.class_frames()]
    frames[0][5, 5, 7] = np.uint64(1 << 63)                            # INT64_MIN in word 7: the resolve does not look at it
    views = [([1, 3, 100, 200][k % 4:] + [1, 3, 100, 200][:k % 4], f) for k, f in enumerate(frames)]
    cases = [(GK.W, GK.H, spp, cs, views)] + [(w, h, 20, 3, _random_views(w, h, n, 60 + w, 8)) for w, h, n in ((1, 1, 5), (5, 3, 3), (9, 17, 3))]
    for width, height, s, c, vs in cases:
        single, batch = unit_read_batch(30, vs, width, height, s, c, gamma, T)
        for v, (chunks, w) in enumerate(vs):
            ref = AW.resolve(w, AW.tile_divisors(chunks, width, height, s, c), gamma, T)
            assert AW.same_bits(batch[v], ref), (width, height, v)
            assert AW.same_bits(single[v], batch[v]), (width, height, v)
        if vs is views:
            assert np.isnan(batch[0][3, 2]).all() and np.isnan(batch[0][12, 10]).all()            # poison is word 6 ...
            assert gamma or not np.isnan(batch[0][5, 5]).any()                                     # ... not word 7 (gamma: sqrt of a negative sum is NaN anyway)
