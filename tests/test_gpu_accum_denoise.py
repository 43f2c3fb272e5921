"""Accumulators as the denoiser's input on the GPU (include/rtw_hip.h rtw_accum_features_*, rtw_accum_noise_*, rtw_guided_filter_device_*,
rtw_accum_filtered_*) against the product's own feature pass, the witnesses tests/accum_denoise_ref.py, tests/features_ref.py and
tests/denoise_ref.py.  Every comparison is on the BITS; NaN pixels are compared as a set.  Tolerance: NONE.
Frames: 48 x 27 (6 x 4 tiles, a ragged last tile row), 64 chunks of one sample, checkpoints 16 / 32 / 48 for the accumulator tests; 24 x 13
with 32 chunks against features_ref; 1 x 1, 5 x 3, 37 x 23, 70 x 41 for the guided filter (tests/test_gpu_denoise.py's frames).
Not reached here: the refusal -2 for an adaptive accumulator whose last adaptive call did not finish.  That state exists only after an
adaptive call has failed half way, and no test provokes such a failure."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import accum_denoise_ref as AR
import accum_words as AW
import denoise_ref as DR
import features_ref as FR
from conftest import CamObj, load_golden
from test_gpu_adaptive import FLOOR, Ad, _same

pytestmark = pytest.mark.gpu

W48, H27, SPP, DEPTH, SEED = 48, 27, 64, 8, 7
FRAMES = [(1, 1), (5, 3), (37, 23), (70, 41)]          # (W, H)
SEEDS = {np.float32: 11, np.float64: 12}


def _tt(T):
    import torch
    return torch.float64 if T is np.float64 else torch.float32


class AcD(Ad):
    """test_gpu_adaptive.Ad plus the entry points of this file, straight on the C ABI (device 0)"""

    def _buf(self, n):
        import torch
        d = torch.full((n,), -7.0, dtype=_tt(self.T), device="cuda:0")
        torch.cuda.synchronize()
        return d

    def stats(self):
        st = self.C.Stats()
        self.C.check(self.L.rtw_stats(C.byref(st)))
        return st

    def features_rc(self, d_ptr, flags=0, seed=None, cam=None, scene=None, spp=None, stream=None):
        P = self._params(flags, 0, 1, seed)
        if spp is not None:
            P.spp = spp
        Cm = self.C.make_camera(cam or self.cam, self.T)
        fn = self.L.rtw_accum_features_f64 if self.T is np.float64 else self.L.rtw_accum_features_f32
        return fn(scene or self.scene, C.byref(Cm), C.byref(P), self.acc, C.c_void_p(d_ptr), C.c_void_p(stream) if stream else None)

    def features(self, flags=0):
        """rtw_accum_features_* -> (raw [H, W, 8], stats)"""
        import torch
        d = self._buf(self.width * self.height * 8)
        self.C.check(self.features_rc(d.data_ptr(), flags))
        st = self.stats()
        torch.cuda.synchronize()
        return d.cpu().numpy().reshape(self.width, self.height, 8).transpose(1, 0, 2), st

    def range_features(self, begin, count, flags=0):
        """rtw_render_features_device_* of the accumulator's render over [begin, begin + count) -> raw [H, W, 8]"""
        import torch
        d = self._buf(self.width * self.height * 8)
        P, Cm = self._params(flags), self.C.make_camera(self.cam, self.T)
        fn = self.L.rtw_render_features_device_f64 if self.T is np.float64 else self.L.rtw_render_features_device_f32
        self.C.check(fn(self.scene, C.byref(Cm), C.byref(P), begin, count, C.c_void_p(d.data_ptr()), None))
        self.stats()
        torch.cuda.synchronize()
        return d.cpu().numpy().reshape(self.width, self.height, 8).transpose(1, 0, 2)

    def noise_rc(self, d_ptr):
        fn = self.L.rtw_accum_noise_f64 if self.T is np.float64 else self.L.rtw_accum_noise_f32
        return fn(self.acc, C.c_void_p(d_ptr), None)

    def noise(self):
        import torch
        d = self._buf(self.width * self.height)
        self.C.check(self.noise_rc(d.data_ptr()))
        torch.cuda.synchronize()
        return d.cpu().numpy().reshape(self.width, self.height).T

    def filtered_rc(self, out, guided, gamma=1, scene=None, cam=None, seed=None, **kw):
        P = self._params(0, 0, gamma, seed)
        Cm = self.C.make_camera(cam or self.cam, self.T)
        D = _dparams(gamma=1 - gamma, **kw)                    # (d->gamma is replaced by p->gamma: hand in the opposite)
        fn = self.L.rtw_accum_filtered_f64 if self.T is np.float64 else self.L.rtw_accum_filtered_f32
        return fn(scene or self.scene, C.byref(Cm), C.byref(P), C.byref(D), self.acc, guided, out.ctypes.data_as(C.c_void_p))

    def filtered(self, guided, gamma=1, **kw):
        out = np.full(self.width * self.height * 3, -7.0, self.T)
        self.C.check(self.filtered_rc(out, guided, gamma, **kw))
        return out.reshape(self.width, self.height, 3).transpose(1, 0, 2)


def _dparams(levels=3, m=1, demodulate=True, gamma=1, sigma_color=1.0, sigma_depth=0.1):
    from rtw_amd import _capi
    return _capi.Denoise(levels, m, 1 if demodulate else 0, gamma, -1, 0, sigma_color, sigma_depth)


def _cfg2():
    g = load_golden("cfg2_random_320x180_64spp_d16_f32", numerics="reference")
    return g["flat"], CamObj(g["cam"])


def _ad48(T, flat=None, cam=None, **kw):
    f, c = _cfg2()
    return AcD(flat or f, cam or c, T, W48, H27, SPP, DEPTH, SEED, n_chunks=SPP, min_chunks=16, check_chunks=16, **kw)


def _ratios_at_16(T, flags=0):
    """the device's own D / M of every tile at checkpoint 16: from the words of an adaptive accumulator whose every tile stopped there
    (a tolerance no tile misses; a plain progressive pass leaves word 7 at 0, so it cannot serve)"""
    from rtw_amd import reference_decisions
    a = _ad48(T)
    try:
        a.run_ok(1e30, flags=flags)
        assert (a.chunks() == 16).all()
        _, D, _, M = reference_decisions(a.words(), W48, H27, 16, 1.0, FLOOR, return_terms=True)
    finally:
        a.close()
    return np.array([d / m for d, m in zip(D, M)])


def _census_ok(ct):
    return (ct == 16).any() and ((ct > 16) & (ct < SPP)).any() and (ct == SPP).any()


def adaptive48(T, flags=0):
    """an adaptive accumulator of the 48 x 27 frame whose tiles stopped at 16, strictly between and never: the tolerance is the middle of a
    gap between two neighbouring ratios of checkpoint 16 (the gaps above the 7th, 5th, 9th, 11th smallest ratio are tried in turn)"""
    r = np.sort(_ratios_at_16(T, flags))
    for rank in (7, 5, 9, 11):
        tol = 0.5 * (r[rank - 1] + r[rank])
        a = _ad48(T)
        a.run_ok(tol, flags=flags)
        if _census_ok(a.chunks()):
            return a, tol
        a.close()
    pytest.fail(f"no candidate tolerance gave tiles at 16, in between and at {SPP}: ratios {r}")


def _assert_same(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: the NaN sets differ ({int(gn.sum())} vs {int(rn.sum())} values)"
    bad = (DR.bits(got) != DR.bits(ref)) & ~gn
    if bad.any():
        where = np.argwhere(bad)[:5]
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} values differ; first: {where.tolist()}; "
                    f"got {[got[tuple(w)] for w in where]} expected {[ref[tuple(w)] for w in where]}")


def _assert_tile_prefixes(a, raw, flags, what):
    """for every distinct c in C_t: the tiles with C_t == c equal those tiles of the feature pass over [0, c)"""
    ct = a.chunks()
    for c in sorted(set(int(x) for x in ct)):
        mk = AR.chunk_mask(ct, c, a.width, a.height)
        assert mk.any()
        _assert_same(raw[mk], a.range_features(0, c, flags)[mk], f"{what}: tiles with C_t == {c}")
    assert not (raw == -7.0).all(axis=2).any()                    # every pixel was written


def _held_samples(a):
    ct = a.chunks()
    return sum(a.npix(t) * int(ct[t]) for t in range(len(ct)))


# ---- a. tile-prefix features ---------------------------------------------------------------------------------------------------------------
@pytest.mark.usefixtures("numerics")
@pytest.mark.parametrize("flags", [0, 4])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_tile_prefix_features_equal_the_feature_pass_of_each_prefix(T, flags):
    a, tol = adaptive48(T, flags)
    try:
        ct = a.chunks()
        assert _census_ok(ct), ct                                  # asserted, not assumed: tiles at 16, strictly between, at 64
        raw, st = a.features(flags)
        _assert_tile_prefixes(a, raw, flags, f"{np.dtype(T).name} flags {flags}")
        assert st.samples == st.segments == _held_samples(a) and st.sphere_tests == st.segments * a.flat["n"] and st.kernel_ms > 0
        # the other scan mode gives the same words (scan flags may differ from the passes')
        _assert_same(a.features(flags ^ 4)[0], raw, "the other scan mode")
    finally:
        a.close()


def test_tile_prefix_features_equal_the_witness(oracle):
    """Float32, the default numerics mode, 24 x 13 (3 x 2 tiles, ragged both ways), 32 chunks of one sample, checkpoints 8 / 16 / 24"""
    from rtw_amd import reference_decisions
    T, W, H, S = np.float32, 24, 13, 32
    flat, cam = _cfg2()
    mk = lambda: AcD(flat, cam, T, W, H, S, DEPTH, SEED, n_chunks=S, min_chunks=8, check_chunks=8)
    b = mk()
    try:
        b.run_ok(1e30)                                             # every tile stops at checkpoint 8: its words carry the half differences
        assert (b.chunks() == 8).all()
        _, D, _, M = reference_decisions(b.words(), W, H, 8, 1.0, FLOOR, return_terms=True)
    finally:
        b.close()
    r = np.sort([d / m for d, m in zip(D, M)])
    a = mk()
    try:
        a.run_ok(0.5 * (r[2] + r[3]))
        ct = a.chunks()
        assert len(set(int(c) for c in ct)) >= 2 and (ct == 8).any(), ct
        with oracle.numerics("reference"):
            it = FR.items(flat, {k: np.asarray(v) for k, v in cam.__dict__.items()}, W, H, S, S, SEED, T, key="cfg2_24x13")
        _assert_same(a.features()[0], AR.tile_prefix_features(it, T, ct, W, H), "against features_ref")
    finally:
        a.close()


# ---- b. uniform accumulators; the refusals that look into an accumulator -------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_uniform_accumulator_and_the_refusals(T):
    import torch
    a = _ad48(T)
    try:
        d = a._buf(W48 * H27 * 8)
        err = a.L.rtw_last_error
        assert a.features_rc(d.data_ptr()) == -2 and b"no chunk interval" in err()                 # nothing held
        assert a.add(3, 8) == 0
        raw, st = a.features()
        _assert_same(raw, a.range_features(3, 8), "the interval [3, 11)")
        assert st.samples == W48 * H27 * 8
        out = np.zeros(W48 * H27 * 3, T)
        assert a.filtered_rc(out, 1) == -2 and b"not adaptive" in err()                            # guided needs word 7
        assert a.noise_rc(d.data_ptr()) == -2 and b"not adaptive" in err()
        # the plain filter of a uniform accumulator: the witness on the device's own resolve and features
        ref = DR.denoise(np.ascontiguousarray(a.resolve(0)), np.ascontiguousarray(raw), T, sigma_color=0.5, gamma=1)
        _assert_same(a.filtered(0, sigma_color=0.5), ref, "the plain filter of a uniform accumulator")
        # not the accumulator's binding: another seed, camera, spp -> -4; other scan flags are fine
        f, c = _cfg2()
        other = CamObj(dict(c.__dict__, lens_radius=np.asarray(c.lens_radius) + np.asarray(c.lens_radius).dtype.type(0.125)))
        assert a.features_rc(d.data_ptr(), seed=SEED + 1) == -4 and b"another render" in err()
        assert a.features_rc(d.data_ptr(), cam=other) == -4 and a.features_rc(d.data_ptr(), spp=SPP - 1) == -4
        assert a.filtered_rc(out, 0, seed=SEED + 1) == -4
        assert a.features_rc(d.data_ptr() + 8) == -2 and b"aligned" in err()
        assert a.features_rc(d.data_ptr(), flags=5) == 0
        # a scene of the other precision -> -4
        b = AcD(f, c, np.float32 if T is np.float64 else np.float64, 8, 5, 2, DEPTH, SEED)
        try:
            assert a.features_rc(d.data_ptr(), scene=b.scene) == -4 and b"precision" in err()
        finally:
            b.close()
        # a second interval -> -2
        assert a.add(20, 4) == 0
        assert a.features_rc(d.data_ptr()) == -2 and b"2 chunk intervals" in err()
        assert a.filtered_rc(out, 0) == -2
        torch.cuda.synchronize()
    finally:
        a.close()


# ---- c. the noise map ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_noise_map_equals_the_witness_on_the_devices_own_words(T):
    a, tol = adaptive48(T)
    try:
        got = a.noise()
        ref = AR.noise_map(a.words(), a.chunks(), W48, H27, SPP, 1, FLOOR, T)
        assert got.dtype == np.dtype(T) and np.isfinite(ref).all() and (ref > 0).any()
        _assert_same(got, ref, f"noise map {np.dtype(T).name}")
    finally:
        a.close()


def unit_noise(words, chunks, width, height, spp, cs, floor, T):
    from rtw_amd import _capi
    L = _capi.lib()
    x = np.concatenate([np.array([width, height, spp, cs, floor, 0, 0, 0], np.float64).view(np.uint64), np.array(chunks, np.float64).view(np.uint64),
                        AW.device_order(words, 8)])
    y = np.full(width * height, -7.0, np.float64)
    fn = L.rtw_unit_f64 if T is np.float64 else L.rtw_unit_f32
    _capi.check(fn(25, 1, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), None, None))
    back = y.astype(T)
    assert AW.same_bits(back.astype(np.float64), y)                   # (every slot holds a value of type T)
    return back.reshape(width, height).T


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_noise_kernel_on_hand_made_words(T):
    for name, words, floor, expect in AR.noise_cases():
        got = unit_noise(words, AR.NCHUNKS, AR.NW, AR.NH, AR.NSPP, AR.NCS, floor, T)
        _assert_same(got, AR.noise_map(words, AR.NCHUNKS, AR.NW, AR.NH, AR.NSPP, AR.NCS, floor, T), name)
        for (i, j), want in expect.items():                            # ... and the expectations spelled out by hand
            assert np.isnan(got[i, j]) if want is None else got[i, j] == np.dtype(T).type(want), (name, i, j)
    # words of every kind at once, random C_t, a frame of several workgroups
    rng = np.random.default_rng(5)
    w = AW.random_words(37, 23, 9)
    chunks = rng.integers(1, 9, size=3 * 5)
    _assert_same(unit_noise(w, chunks, 37, 23, 20, 3, 0.03, T), AR.noise_map(w, chunks, 37, 23, 20, 3, 0.03, T), "random words")


# ---- d. the guided filter ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frame(W, H, T):
    image, feat = DR.handmade(H, W, T, SEEDS[T])
    noise = AR.special_noise(H, W, T, SEEDS[T] + 100)
    for x in (image, feat, noise):
        x.setflags(write=False)
    return image, feat, noise


def _lib_layout(a):
    return np.array(a.transpose(1, 0, 2) if a.ndim == 3 else a.T, order="C", copy=True)


class GuidedFrame:
    def __init__(self, W, H, T):
        import torch
        from rtw_amd import _capi
        self.L, self.T, self.W, self.H = _capi.lib(), T, W, H
        image, feat, noise = _frame(W, H, T)
        self.img, self.feat, self.noise = (torch.from_numpy(_lib_layout(x)).to("cuda:0") for x in (image, feat, noise))
        self.work_elems = int(self.L.rtw_denoise_work_bytes(W, H, np.dtype(T).itemsize)) // np.dtype(T).itemsize
        torch.cuda.synchronize()

    def workspace(self, poison=False):
        import torch
        w = torch.zeros(self.work_elems, dtype=_tt(self.T), device="cuda:0")
        if poison:
            w.fill_(float("nan"))
        return w

    def run(self, work=None, stream=None, **kw):
        import torch
        from rtw_amd import _capi
        work = self.workspace() if work is None else work
        out = torch.full((self.W * self.H * 3,), -7.0, dtype=_tt(self.T), device="cuda:0")
        torch.cuda.synchronize()
        D = _dparams(**kw)
        fn = self.L.rtw_guided_filter_device_f64 if self.T is np.float64 else self.L.rtw_guided_filter_device_f32
        _capi.check(fn(C.byref(D), self.W, self.H, C.c_void_p(self.img.data_ptr()), C.c_void_p(self.feat.data_ptr()), C.c_void_p(self.noise.data_ptr()),
                       C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr()), C.c_void_p(stream.cuda_stream) if stream is not None else None))
        self._keep = work
        if stream is None:
            torch.cuda.synchronize()
        return out

    def image(self, out):
        return out.cpu().numpy().reshape(self.W, self.H, 3).transpose(1, 0, 2)


@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_guided_frames_equal_the_witness(T, W, H):
    image, feat, noise = _frame(W, H, T)
    dev = GuidedFrame(W, H, T)
    work = dev.workspace()
    for levels in (1, 3, 5):
        for demodulate in (True, False):
            for gamma in (0, 1):
                kw = dict(levels=levels, demodulate=demodulate, gamma=gamma)
                ref = AR.guided(image, feat, noise, T, **kw)
                _assert_same(dev.image(dev.run(work=work, **kw)), ref, f"{np.dtype(T).name} {W}x{H} {kw}")
    if W * H >= 12:
        assert np.isnan(ref[~np.isfinite(noise)]).all() and np.isfinite(ref).any()
    # sigma_color and m reach the kernels
    for kw in (dict(sigma_color=0.25), dict(sigma_color=8.0, m=3)):
        _assert_same(dev.image(dev.run(work=work, **kw)), AR.guided(image, feat, noise, T, **kw), str(kw))


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_guided_poisoned_workspace_and_two_streams(T):
    import torch
    W, H = 70, 41
    image, feat, noise = _frame(W, H, T)
    dev = GuidedFrame(W, H, T)
    ref3, ref5 = AR.guided(image, feat, noise, T, levels=3), AR.guided(image, feat, noise, T, levels=5)
    _assert_same(dev.image(dev.run(work=dev.workspace(poison=True), levels=3)), ref3, "a workspace full of NaN")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    w1, w2 = dev.workspace(), dev.workspace(poison=True)
    torch.cuda.synchronize()
    o1 = dev.run(work=w1, stream=s1, levels=3)
    o2 = dev.run(work=w2, stream=s2, levels=5)
    torch.cuda.synchronize()
    _assert_same(dev.image(o1), ref3, "stream 1")
    _assert_same(dev.image(o2), ref5, "stream 2")


# ---- e. the one call; f. the accumulator is untouched ------------------------------------------------------------------------------------------
def _assert_one_call_is_the_witness(a, what):
    T = a.T
    raw = np.ascontiguousarray(a.resolve(0))
    feat = np.ascontiguousarray(a.features()[0])
    noise = np.ascontiguousarray(a.noise())
    for gamma in (0, 1):
        _assert_same(a.filtered(1, gamma), AR.guided(raw, feat, noise, T, gamma=gamma), f"{what}: guided, gamma {gamma}")
        _assert_same(a.filtered(0, gamma, sigma_color=0.5), DR.denoise(raw, feat, T, sigma_color=0.5, gamma=gamma), f"{what}: plain, gamma {gamma}")
    _assert_same(a.filtered(1, 1, levels=2, demodulate=False, sigma_color=2.0), AR.guided(raw, feat, noise, T, levels=2, demodulate=False, sigma_color=2.0),
                 f"{what}: guided, other parameters")
    st = a.stats()                                                 # the feature pass's record
    assert st.samples == st.segments == _held_samples(a)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_one_call_equals_the_witness_and_leaves_the_accumulator_alone(T):
    a, tol = adaptive48(T)
    try:
        words, ct, info = a.words().copy(), a.chunks().copy(), a.ainfo()
        _assert_one_call_is_the_witness(a, np.dtype(T).name)
        assert _same(a.words(), words) and np.array_equal(a.chunks(), ct) and a.ainfo() == info
        # a refinement afterwards equals a fresh run at the smaller tolerance
        a.run_ok(0.5 * tol)
        b = _ad48(T)
        try:
            b.run_ok(0.5 * tol)
            assert _same(a.words(), b.words()) and np.array_equal(a.chunks(), b.chunks())
            _assert_same(a.features()[0], b.features()[0], "features after a refinement")
        finally:
            b.close()
    finally:
        a.close()


def test_view_1_of_a_batched_adaptive_run():
    import test_gpu_accum_batch as AB
    T = np.float32
    flat, cam = _cfg2()
    cam2 = CamObj(dict(cam.__dict__, lens_radius=np.asarray(cam.lens_radius) + np.float32(0.125)))
    r = np.sort(_ratios_at_16(T))
    vs = [AcD(flat, cm, T, W48, H27, SPP, DEPTH, sd, n_chunks=SPP, min_chunks=16, check_chunks=16) for cm, sd in ((cam, SEED), (cam2, SEED + 5))]
    try:
        AB.ok(AB.batch_adapt(vs, 0.5 * (r[6] + r[7])), vs[0])
        a = vs[1]
        assert len(set(int(c) for c in a.chunks())) >= 2
        _assert_tile_prefixes(a, a.features()[0], 0, "view 1")
        _assert_one_call_is_the_witness(a, "view 1 of a batch")
        out = np.zeros(W48 * H27 * 3, T)
        assert a.filtered_rc(out, 1, cam=cam, seed=SEED) == -4          # view 0's camera and seed are not view 1's binding
    finally:
        AB.close(vs)


# ---- g. a scene that is read from global memory ---------------------------------------------------------------------------------------------
_PROBE = """
import sys
sys.path[:0] = [{tests!r}, {root!r}, {oracle!r}]
import torch
torch.cuda.init()                       # (two HIP runtimes in one process: torch's goes first, tests/conftest.py)
import numpy as np
import big_scenes as BS
import test_gpu_accum_denoise as G
T = np.float32
a = G.AcD(BS.scene(T), BS.cameras(T)[0], T, 48, 27, 32, 8, 7, n_chunks=32, min_chunks=8, check_chunks=8)
a.run_ok(float(sys.argv[1]))
ct = a.chunks()
print("@features", file=sys.stderr, flush=True)
raw, st = a.features()
print("@end", file=sys.stderr, flush=True)
G._assert_tile_prefixes(a, raw, 0, "1600 spheres")
assert st.samples == G._held_samples(a)
print("distinct", len(set(int(c) for c in ct)))
a.close()
"""


def test_the_tiled_global_scene_instance(oracle):
    """tests/big_scenes.py's 1600-sphere Float32 scene (not staged in LDS), its adaptive frame and tolerance; a fresh process, because
    the RTW_DEBUG aid is read once per process: the line between the marks names the tiled global-scene instance"""
    import big_scenes as BS
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    with oracle.numerics("reference"):
        case = BS.adaptive_case(oracle, np.float32)
    code = _PROBE.format(tests=tests, root=root, oracle=os.path.join(root, "oracle"))
    env = dict(os.environ, RTW_ENABLE_TEST_AIDS="1", RTW_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", code, repr(case["tol"])], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert int(r.stdout.split("distinct")[1].split()[0]) >= 2, r.stdout
    section = r.stderr.split("@features")[1].split("@end")[0]
    lines = BS.parse_instance_lines(section)
    assert len(lines) == 1, section[-500:]
    inst = lines[0][0]
    assert (inst.kernel, inst.lds_scene, inst.mfma, inst.accum, inst.adapt, inst.batch, inst.cull) == ("features", 0, 1, 1, 1, 0, 0), inst
    # the plain feature pass keeps saying accum=0 adapt=0
    rest = BS.parse_instance_lines(r.stderr.split("@end")[1])
    assert rest and all(i.kernel == "features" and i.accum == 0 and i.adapt == 0 for i, _, _ in rest)


# ---- h. the Python layer ------------------------------------------------------------------------------------------------------------------------
def test_the_python_layer(rtw):
    """the package's own random-spheres scene at 64 x 36, 48 chunks of one sample, checkpoints 16 / 32"""
    import importlib
    from rtw_amd._capi import RtwError
    T, W, H, S = np.float32, 64, 36, 48
    scene, cam = rtw.scene_random_spheres(elem_type=T), rtw.t_cam1(elem_type=T)
    kw = dict(dark_floor=FLOOR, min_chunks=16, check_chunks=16, depth=DEPTH, seed=3)
    with rtw.AdaptiveRenderer(scene, cam, W, S, **kw) as ar:
        ar.run(0.05)
        ct = ar.tile_chunks().T.reshape(-1)
        assert len(set(int(c) for c in ct)) >= 2, ct
        raw, feat, noise = np.ascontiguousarray(ar.image(gamma=False)), ar.features(), ar.noise()
        assert feat["raw"].shape == (H, W, 8) and feat["coverage"].shape == (H, W) and noise.shape == (H, W) and noise.dtype == T
        _assert_same(noise, AR.noise_map(ar.read_pixels(), ct, W, H, S, 1, FLOOR, T), "AdaptiveRenderer.noise")
        fr = np.ascontiguousarray(feat["raw"])
        for c in sorted(set(int(x) for x in ct)):                    # the features of each tile are those of the chunks it holds
            mk = AR.chunk_mask(ct, c, W, H)
            ref = rtw.render_features(scene, cam, W, S, seed=3, chunks=(0, c))["raw"]
            _assert_same(fr[mk], np.ascontiguousarray(ref)[mk], f"AdaptiveRenderer.features, C_t == {c}")
        sc = importlib.import_module("rtw_amd.denoise").GUIDED_SIGMA_COLOR
        guided = ar.denoised()
        _assert_same(guided, AR.guided(raw, fr, np.ascontiguousarray(noise), T, sigma_color=sc), "AdaptiveRenderer.denoised")
        _assert_same(ar.denoised(guided=False, gamma=False, levels=2), DR.denoise(raw, fr, T, levels=2, gamma=0), "denoised(guided=False)")
        with pytest.raises(RtwError):
            ar.add(1)
    img, spp_map, info = rtw.render_adaptive_denoised(scene, cam, W, S, tolerance=0.05, **kw)
    _assert_same(img, guided, "render_adaptive_denoised")
    assert spp_map.shape == (H, W) and info["n_tiles"] == 40
    with rtw.ProgressiveRenderer(scene, cam, W, S, depth=DEPTH, seed=3) as pr:
        pr.add_range(3, 8)
        f = pr.features()
        _assert_same(np.ascontiguousarray(f["raw"]), np.ascontiguousarray(rtw.render_features(scene, cam, W, S, seed=3, chunks=(3, 8))["raw"]), "ProgressiveRenderer.features")
        _assert_same(pr.denoised(gamma=False), DR.denoise(np.ascontiguousarray(pr.image(gamma=False)), np.ascontiguousarray(f["raw"]), T, gamma=0),
                     "ProgressiveRenderer.denoised")
        pr.add_range(20, 2)
        with pytest.raises(RtwError) as e:
            pr.features()
        assert e.value.code == -2
    # the accumulators of the batch renderers are accepted view by view
    cams, seeds = [cam, rtw.t_default_cam(elem_type=T)], [3, 11]
    with rtw.AdaptiveBatchRenderer(scene, cams, W, S, dark_floor=FLOOR, min_chunks=16, check_chunks=16, depth=DEPTH, seeds=seeds) as ab:
        ab.run(0.05)
        with rtw.AdaptiveRenderer(scene, cams[1], W, S, dark_floor=FLOOR, min_chunks=16, check_chunks=16, depth=DEPTH, seed=seeds[1]) as one:
            one.run(0.05)
            _assert_same(ab.denoised(1), one.denoised(), "AdaptiveBatchRenderer.denoised(1)")
            _assert_same(ab.denoised(1, guided=False, gamma=False), one.denoised(guided=False, gamma=False), "AdaptiveBatchRenderer.denoised(1, guided=False)")
        _assert_same(ab.denoised(0), guided, "AdaptiveBatchRenderer.denoised(0)")
    with rtw.ProgressiveBatchRenderer(scene, cams, W, S, depth=DEPTH, seeds=seeds) as pb:
        pb.add_range(3, 8)
        with rtw.ProgressiveRenderer(scene, cams[1], W, S, depth=DEPTH, seed=seeds[1]) as one:
            one.add_range(3, 8)
            _assert_same(pb.denoised(1, gamma=False), one.denoised(gamma=False), "ProgressiveBatchRenderer.denoised(1)")
