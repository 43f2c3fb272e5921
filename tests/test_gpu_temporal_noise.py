"""The temporal moments on the GPU (include/rtw_hip.h rtw_history_moments_*, rtw_history_noise_device_*, rtw_render_path_guided_*)
against the witness tests/temporal_noise_ref.py.  Every comparison is on the BITS -- the image, the three planes of the state, the moment
plane and the noise map; NaN values are compared as a set.  Tolerance: NONE.
Frames (W x H): 1x1; 3x2 (smaller than the window of every radius); 70x40 (2800 pixels: 11 workgroups, the last one partial; H is no multiple
of 64, so waves straddle columns); 64x36.  tests/test_temporal_noise_ref.py shows that the committed seeds reach every regime of the two
definitions on the two larger frames."""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_ref as DR
import temporal_noise_ref as NR
import temporal_ref as TR

pytestmark = pytest.mark.gpu

SIZES = NR.SIZES
STEP_KW = [dict(m=1), dict(m=0, demodulate=False, gamma=0)]
NOISE_KW = [dict(radius=r, m=m, min_len=ml) for r in (1, 3) for m in (0, 1) for ml in (1.0, 4.0)] + [dict(NR.NOISE_DEFAULTS)]


@functools.lru_cache(maxsize=None)
def _sequence(size, T):
    W, H = size
    cams, frames, state0, moment0, cam0 = NR.handmade_sequence(H, W, T, NR.SEEDS[T], 3)
    for image, feat in frames:
        image.setflags(write=False)
        feat.setflags(write=False)
    for a in list(state0.values()) + [moment0]:
        a.setflags(write=False)
    return cams, frames, state0, moment0, cam0


@functools.lru_cache(maxsize=None)
def _witness(size, T, first, kw):
    """step 0 of the size's sequence with moments: a first frame, or on the hand-made previous state -> (out, state, M)"""
    cams, frames, state0, moment0, cam0 = _sequence(size, T)
    return NR.step_moments(*frames[0], cams[0], T, None if first else state0, None if first else moment0, None if first else cam0, **dict(kw))


def _key(kw):
    return tuple(sorted(kw.items()))


def _lib_layout(a):
    return np.array(np.swapaxes(a, 0, 1), order="C", copy=True)


def _sfx(T):
    return "f64" if T is np.float64 else "f32"


def _tparams(**kw):
    from rtw_amd import _capi
    v = dict(TR.DEFAULTS)
    v.update(kw)
    return _capi.Temporal(v["m"], 1 if v["demodulate"] else 0, v["gamma"], -1, (C.c_int32 * 2)(0, 0), v["sigma_depth"], v["min_weight"], v["history_max"])


def _nparams(**kw):
    from rtw_amd import _capi
    v = dict(NR.NOISE_DEFAULTS)
    v.update(kw)
    return _capi.TemporalNoise(v["radius"], v["m"], -1, (C.c_int32 * 3)(0, 0, 0), v["sigma_depth"], v["min_len"])


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def step_host(image, feat, cam, T, state=None, moment=None, cam_prev=None, noise=None, **kw):
    """rtw_history_moments_* on [H, W, .] arrays -> (out, next state, M, rho); the outputs start poisoned"""
    from rtw_amd import _capi
    L = _capi.lib()
    H, W = image.shape[:2]
    img, ft = _lib_layout(image), _lib_layout(feat)
    out, rho = np.full((W, H, 3), -7.0, T), np.full((W, H), -7.0, T)
    nxt, mom = np.full(TR.state_elems(H, W, T), -7.0, T), np.full(NR.moment_elems(H, W, T), -7.0, T)
    sp = TR.pack_state(state, T) if state is not None else None
    mp = NR.pack_moment(moment, T) if moment is not None else None
    Cm = _capi.make_camera(cam, T)
    Cp = C.byref(_capi.make_camera(cam_prev, T)) if cam_prev is not None else None
    _capi.check(getattr(L, "rtw_history_moments_" + _sfx(T))(C.byref(_tparams(**kw)), C.byref(_nparams(**(noise or {}))), C.byref(Cm), Cp, W, H, _ptr(img), _ptr(ft), _ptr(sp),
                                                              _ptr(mp), _ptr(nxt), _ptr(mom), _ptr(out), _ptr(rho)))
    return np.swapaxes(out, 0, 1), TR.unpack_state(nxt, H, W), NR.unpack_moment(mom, H, W), np.swapaxes(rho, 0, 1)


class DeviceFrames:
    """the frames of a sequence, a previous state and its moment plane as torch tensors on cuda:0, and the device entry points on them"""

    def __init__(self, frames, T, state0=None, moment0=None):
        import torch
        from rtw_amd import _capi
        self.torch, self.L, self.T = torch, _capi.lib(), T
        self.H, self.W = frames[0][0].shape[:2]
        self.n = self.W * self.H
        self.host = [(_lib_layout(i), _lib_layout(f)) for i, f in frames]
        self.dev = [(torch.from_numpy(i).to("cuda:0"), torch.from_numpy(f).to("cuda:0")) for i, f in self.host]
        self.n_state, self.n_mom = TR.state_elems(self.H, self.W, T), NR.moment_elems(self.H, self.W, T)
        eb = np.dtype(T).itemsize
        assert self.n_state * eb == self.L.rtw_temporal_state_bytes(self.W, self.H, eb) and self.n_mom * eb == self.L.rtw_history_moment_bytes(self.W, self.H, eb)
        self.host0 = [TR.pack_state(state0, T), NR.pack_moment(moment0, T)] if state0 is not None else None
        self.state0, self.moment0 = [torch.from_numpy(a).to("cuda:0") for a in self.host0] if state0 is not None else (None, None)
        torch.cuda.synchronize()

    def buffers(self, poison=-7.0):
        """-> (next state, next moment plane, out, noise map of the ROUNDED size), filled with `poison`"""
        dt = self.dev[0][0].dtype
        return tuple(self.torch.full((k,), poison, dtype=dt, device="cuda:0") for k in (self.n_state, self.n_mom, self.n * 3, self.n_mom))

    def _cams(self, cam, cam_prev):
        from rtw_amd import _capi
        return _capi.make_camera(cam, self.T), (C.byref(_capi.make_camera(cam_prev, self.T)) if cam_prev is not None else None)

    def step(self, k, cam, state=None, moment=None, cam_prev=None, bufs=None, **kw):
        """rtw_history_moments_device_* on frame k -> (next state, next moments, out, the untouched map buffer), synchronised"""
        from rtw_amd import _capi
        bufs = self.buffers() if bufs is None else bufs
        self.torch.cuda.synchronize()                              # the fills ran on torch's stream
        Cm, Cp = self._cams(cam, cam_prev)
        img, feat = self.dev[k]
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _capi.check(getattr(self.L, "rtw_history_moments_device_" + _sfx(self.T))(C.byref(_tparams(**kw)), C.byref(Cm), Cp, self.W, self.H, vp(img), vp(feat), vp(state),
                                                                                   vp(moment), vp(bufs[0]), vp(bufs[1]), vp(bufs[2]), None))
        self.torch.cuda.synchronize()
        return bufs

    def plain_step(self, k, cam, state=None, cam_prev=None, **kw):
        """rtw_temporal_device_* on frame k -> (next state, out)"""
        from rtw_amd import _capi
        nxt, _, out, _ = self.buffers()
        self.torch.cuda.synchronize()
        Cm, Cp = self._cams(cam, cam_prev)
        img, feat = self.dev[k]
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _capi.check(getattr(self.L, "rtw_temporal_device_" + _sfx(self.T))(C.byref(_tparams(**kw)), C.byref(Cm), Cp, self.W, self.H, vp(img), vp(feat), vp(state), vp(nxt), vp(out),
                                                                           None))
        self.torch.cuda.synchronize()
        return nxt, out

    def noise(self, state, moment, rho, **nk):
        """rtw_history_noise_device_* -> rho, synchronised"""
        from rtw_amd import _capi
        self.torch.cuda.synchronize()
        _capi.check(getattr(self.L, "rtw_history_noise_device_" + _sfx(self.T))(C.byref(_nparams(**nk)), self.W, self.H, C.c_void_p(state.data_ptr()), C.c_void_p(moment.data_ptr()),
                                                                                 C.c_void_p(rho.data_ptr()), None))
        self.torch.cuda.synchronize()
        return rho

    def image(self, out):
        return out.cpu().numpy().reshape(self.W, self.H, 3).transpose(1, 0, 2)

    def state(self, nxt):
        return TR.unpack_state(nxt.cpu().numpy(), self.H, self.W)

    def plane(self, t):
        return NR.unpack_moment(t.cpu().numpy(), self.H, self.W)

    def inputs_unchanged(self):
        same = all(np.array_equal(DR.bits(t.cpu().numpy()), DR.bits(a)) for dev, host in zip(self.dev, self.host) for t, a in zip(dev, host))
        if self.host0 is not None:
            same = same and all(np.array_equal(DR.bits(t.cpu().numpy()), DR.bits(a)) for t, a in zip((self.state0, self.moment0), self.host0))
        return same


def _assert_same(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: the NaN sets differ ({int(gn.sum())} vs {int(rn.sum())} values)"
    bad = (DR.bits(got) != DR.bits(ref)) & ~gn
    if bad.any():
        where = np.argwhere(bad)[:5]
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} values differ; first index: {where.tolist()}; "
                    f"got {[got[tuple(w)] for w in where]} expected {[ref[tuple(w)] for w in where]}")


def _assert_step(got, ref, what):
    """(out, state, M) triples: the image, the three planes, the moment plane"""
    _assert_same(got[0], ref[0], what + ": image")
    for k in ("E", "G", "L"):
        _assert_same(got[1][k], ref[1][k], f"{what}: state plane {k}")
    _assert_same(got[2], ref[2], what + ": moment plane")


# ---- 1. every frame, precision and parameter set through both entry points -------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_device_forms_equal_the_witness(T, size):
    cams, frames, state0, moment0, cam0 = _sequence(size, T)
    dev = DeviceFrames(frames[:1], T, state0, moment0)
    bufs = dev.buffers()
    for first in (True, False):
        for kw in STEP_KW:
            ref = _witness(size, T, first, _key(kw))
            nxt, mom, out, rho = dev.step(0, cams[0], None if first else dev.state0, None if first else dev.moment0, None if first else cam0, bufs=bufs, **kw)
            _assert_step((dev.image(out), dev.state(nxt), dev.plane(mom)), ref, f"{np.dtype(T).name} {size} first={first} {kw}")
            # the image and the state are rtw_temporal_device_*'s on the bits
            pn, po = dev.plain_step(0, cams[0], None if first else dev.state0, None if first else cam0, **kw)
            assert np.array_equal(DR.bits(pn.cpu().numpy()[:9 * dev.n]), DR.bits(nxt.cpu().numpy()[:9 * dev.n])) and np.array_equal(DR.bits(po.cpu().numpy()), DR.bits(out.cpu().numpy()))
            for nk in NOISE_KW:
                dev.noise(nxt, mom, rho, **nk)
                _assert_same(dev.plane(rho), NR.noise_map(ref[1], ref[2], T, **nk), f"{np.dtype(T).name} {size} first={first} {kw} map {nk}")
    assert dev.inputs_unchanged()


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_host_form_equals_the_witness(T, size):
    cams, frames, state0, moment0, cam0 = _sequence(size, T)
    for first in (True, False):
        for kw, nk in ((STEP_KW[0], NOISE_KW[-1]), (STEP_KW[1], NOISE_KW[1]), (STEP_KW[0], NOISE_KW[6])):
            ref = _witness(size, T, first, _key(kw))
            got = step_host(*frames[0], cams[0], T, None if first else state0, None if first else moment0, None if first else cam0, noise=nk, **kw)
            _assert_step(got[:3], ref, f"host {np.dtype(T).name} {size} first={first} {kw}")
            _assert_same(got[3], NR.noise_map(ref[1], ref[2], T, **nk), f"host {np.dtype(T).name} {size} first={first} map {nk}")


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_parameters_reach_the_kernels(T):
    size = (70, 40)
    cams, frames, state0, moment0, cam0 = _sequence(size, T)
    dev = DeviceFrames(frames[:1], T, state0, moment0)
    base = _witness(size, T, False, _key(dict(m=1)))
    base_map = NR.noise_map(base[1], base[2], T)
    for kw in (dict(sigma_depth=0.002), dict(min_weight=0.9), dict(history_max=3.5)):
        ref = NR.step_moments(*frames[0], cams[0], T, state0, moment0, cam0, **kw)
        assert not TR.same_bits(ref[2], base[2]), kw
        nxt, mom, out, rho = dev.step(0, cams[0], dev.state0, dev.moment0, cam0, **kw)
        _assert_step((dev.image(out), dev.state(nxt), dev.plane(mom)), ref, f"device {kw}")
    nxt, mom, out, rho = dev.step(0, cams[0], dev.state0, dev.moment0, cam0)
    for nk in (dict(sigma_depth=0.002), dict(min_len=2.5), dict(min_len=100.0), dict(radius=1), dict(m=7)):
        ref = NR.noise_map(base[1], base[2], T, **dict(NR.NOISE_DEFAULTS, **nk))
        assert not TR.same_bits(ref, base_map), nk
        _assert_same(dev.plane(dev.noise(nxt, mom, rho, **dict(NR.NOISE_DEFAULTS, **nk))), ref, f"map {nk}")


# ---- 2. a chain of three steps on the device --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(70, 40), (64, 36)])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_three_step_chain(T, size):
    cams, frames, state0, moment0, cam0 = _sequence(size, T)
    dev = DeviceFrames(frames, T, state0, moment0)
    for start in ("first frame", "hand-made state"):
        ref_st, ref_mo, ref_cam = (None, None, None) if start == "first frame" else (state0, moment0, cam0)
        d_st, d_mo = (None, None) if start == "first frame" else (dev.state0, dev.moment0)
        long_history = False
        for k in range(3):
            ref_out, ref_st, ref_mo = NR.step_moments(*frames[k], cams[k], T, ref_st, ref_mo, ref_cam)
            d_st, d_mo, out, rho = dev.step(k, cams[k], d_st, d_mo, ref_cam)
            what = f"{np.dtype(T).name} {size} {start}, step {k}"
            _assert_step((dev.image(out), dev.state(d_st), dev.plane(d_mo)), (ref_out, ref_st, ref_mo), what)
            _assert_same(dev.plane(dev.noise(d_st, d_mo, rho, min_len=3.0)), NR.noise_map(ref_st, ref_mo, T, **dict(NR.NOISE_DEFAULTS, min_len=3.0)), what + ": map")
            ref_cam = cams[k]
            long_history = long_history or bool((ref_st["L"] >= 3).any())
        assert long_history                                  # (the temporal branch on moments the device itself accumulated)
    assert dev.inputs_unchanged()


# ---- 3. poisoned outputs change nothing; nothing behind the last element is written -----------------------------------------------------------
@pytest.mark.parametrize("size", [(3, 2), (70, 40)])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_poisoned_outputs_change_nothing(T, size):
    cams, frames, state0, moment0, cam0 = _sequence(size, T)
    dev = DeviceFrames(frames[:1], T, state0, moment0)
    n = dev.n
    for first in (True, False):
        ref = _witness(size, T, first, _key(dict(m=1)))
        ref_map = NR.noise_map(ref[1], ref[2], T)
        for poison in (float("nan"), float("inf"), 1e30):
            nxt, mom, out, rho = dev.step(0, cams[0], None if first else dev.state0, None if first else dev.moment0, None if first else cam0, bufs=dev.buffers(poison))
            _assert_step((dev.image(out), dev.state(nxt), dev.plane(mom)), ref, f"poison {poison} first={first}")
            dev.noise(nxt, mom, rho)
            _assert_same(dev.plane(rho), ref_map, f"poison {poison} first={first}: map")
            # every byte of the M and the map buffer: the first W*H elements are the witness's, the padding up to the rounded size is not the kernels' to write
            pad = np.full(dev.n_mom - n, poison, T)
            assert np.array_equal(DR.bits(mom.cpu().numpy()[:n]), DR.bits(NR.pack_moment(ref[2], T)[:n])) and np.array_equal(DR.bits(mom.cpu().numpy()[n:]), DR.bits(pad))
            assert np.array_equal(DR.bits(rho.cpu().numpy()[:n]), DR.bits(_lib_layout(ref_map).reshape(-1))) and np.array_equal(DR.bits(rho.cpu().numpy()[n:]), DR.bits(pad))
            assert np.array_equal(DR.bits(nxt.cpu().numpy()[9 * n:]), DR.bits(np.full(dev.n_state - 9 * n, poison, T)))
    assert dev.n_mom > n or not (size == (3, 2) and T is np.float32)         # (6 binary32 elements: 8 bytes of padding to look at)
    assert dev.inputs_unchanged()


# ---- 4. the sequence call equals its parts ---------------------------------------------------------------------------------------------------
_STAT_KEYS = ("samples", "segments", "sphere_tests", "n_chunks", "grid_blocks", "block_threads")


def _orbit(rtw, T, n, radius=1.5, arc=0.5):
    cams = []
    for v in range(n):
        phi = arc * v / max(n - 1, 1)
        cams.append(rtw.default_camera(lookfrom=(radius * np.sin(phi), 0.4, -1 + radius * np.cos(phi)), lookat=(0, 0, -1), vfov=60, aperture=0, elem_type=T))
    return cams


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_render_sequence_guided_equals_its_parts(rtw, T):
    """3 views of 64x36 at 1 spp over the two-sphere scene: view v against the chain of the single DEVICE calls (the step with moments, the
    map, the guided filter) over the product's own renders and features, on the bits; the map of each view against the witness"""
    import torch
    W, H, N = 64, 36, 3
    scene, cams, seeds = rtw.scene_2_spheres(elem_type=T), _orbit(rtw, T, N), [21, 22, 23]
    tkw = dict(normal_power_log2=1, sigma_depth=0.2, min_weight=0.125, history_max=6.0)
    nkw = dict(radius=2, normal_power_log2=1, sigma_depth=0.1, min_len=2.0)
    dkw = dict(levels=2, sigma_color=1.5)
    rtw.render_batch(scene, cams, W, 1, seed=seeds, gamma=False)
    batch_stats = {k: rtw.last_stats()[k] for k in _STAT_KEYS}
    assert batch_stats["samples"] == N * W * H
    dt = torch.float64 if T is np.float64 else torch.float32
    eb = np.dtype(T).itemsize
    full = lambda k: torch.full((k,), float("nan"), dtype=dt, device="cuda:0")
    for gamma in (True, False):
        got = rtw.render_sequence(scene, cams, W, 1, seeds=seeds, denoise=dkw, guided=nkw, gamma=gamma, **tkw)
        assert got.shape == (N, H, W, 3) and got.dtype == T and np.isfinite(got).all()
        assert {k: rtw.last_stats()[k] for k in _STAT_KEYS} == batch_stats         # rtw_stats: the render's record
        st, mo = [full(rtw.temporal_state_bytes(W, H, T) // eb) for _ in range(2)], [full(rtw.temporal_moment_bytes(W, H, T) // eb) for _ in range(2)]
        acc, rho, flt, work = full(W * H * 3), full(W * H), full(W * H * 3), torch.zeros(rtw.denoise_work_bytes(W, H, T) // eb, dtype=dt, device="cuda:0")
        wit, cam_prev, used_both = None, None, [False, False]
        for v in range(N):
            lin = rtw.render(scene, cams[v], W, 1, seed=seeds[v], gamma=False)
            feat = rtw.render_features(scene, cams[v], W, 1, seed=seeds[v])["raw"]
            d_lin, d_feat = torch.from_numpy(_lib_layout(lin)).to("cuda:0"), torch.from_numpy(_lib_layout(feat)).to("cuda:0")
            torch.cuda.synchronize()
            rtw.temporal_step_moments_into(acc.data_ptr(), st[v & 1].data_ptr(), mo[v & 1].data_ptr(), d_lin.data_ptr(), d_feat.data_ptr(), cams[v], W, H,
                                           d_state_prev_ptr=st[(v & 1) ^ 1].data_ptr() if v else None, d_moment_prev_ptr=mo[(v & 1) ^ 1].data_ptr() if v else None,
                                           cam_prev=cam_prev, elem_type=T, gamma=False, **tkw)
            rtw.temporal_noise_into(rho.data_ptr(), st[v & 1].data_ptr(), mo[v & 1].data_ptr(), W, H, elem_type=T, **nkw)
            rtw.denoise_guided_into(flt.data_ptr(), acc.data_ptr(), d_feat.data_ptr(), rho.data_ptr(), work.data_ptr(), W, H, elem_type=T, gamma=gamma, **dkw)
            torch.cuda.synchronize()
            part = flt.cpu().numpy().reshape(W, H, 3).transpose(1, 0, 2)
            _assert_same(got[v], part, f"{np.dtype(T).name} view {v} gamma={gamma}")
            wit = NR.step_moments(np.ascontiguousarray(lin), np.ascontiguousarray(feat), cams[v], T, None if v == 0 else wit[1], None if v == 0 else wit[2], cam_prev, m=1,
                                  sigma_depth=0.2, min_weight=0.125, history_max=6.0, gamma=0)
            ref_map = NR.noise_map(wit[1], wit[2], T, radius=2, m=1, sigma_depth=0.1, min_len=2.0)
            _assert_same(rho.cpu().numpy().reshape(W, H).T, ref_map, f"view {v}: the map against the witness")
            long_ = wit[1]["L"] >= 2
            used_both = [used_both[0] or bool(long_.any()), used_both[1] or bool((~long_ & ~np.isnan(ref_map)).any())]
            cam_prev = cams[v]
        assert all(used_both)                               # (both branches of the map fed the filter)
    plain = rtw.render_sequence(scene, cams, W, 1, seeds=seeds, denoise=dkw, **tkw)
    assert not TR.same_bits(plain, got)                     # (the guided call is not the plain one)


# ---- 5. the Python layer ---------------------------------------------------------------------------------------------------------------------
def test_python_layer(rtw):
    import torch
    T = np.float32
    size = (70, 40)
    W, H = size
    cams, frames, state0, moment0, cam0 = _sequence(size, T)
    ref = _witness(size, T, False, _key(dict(m=1)))
    from rtw_amd.features import split
    out, nxt, mom, rho = rtw.temporal_step_moments(*frames[0], cams[0], TR.pack_state(state0, T), NR.pack_moment(moment0, T), cam0)
    _assert_step((out, TR.unpack_state(nxt, H, W), NR.unpack_moment(mom, H, W)), ref, "temporal_step_moments")
    _assert_same(rho, NR.noise_map(ref[1], ref[2], T), "temporal_step_moments: map")
    assert rho.shape == (H, W) and mom.shape == (NR.moment_elems(H, W, T),)
    out, nxt, mom, rho = rtw.temporal_step_moments(frames[0][0], split(frames[0][1]), cams[0], normal_power_log2=0, demodulate=False, gamma=False,
                                                   noise=dict(radius=3, normal_power_log2=0, min_len=1.0))
    ref1 = _witness(size, T, True, _key(STEP_KW[1]))
    _assert_step((out, TR.unpack_state(nxt, H, W), NR.unpack_moment(mom, H, W)), ref1, "temporal_step_moments keywords, first frame")
    _assert_same(rho, NR.noise_map(ref1[1], ref1[2], T, radius=3, m=0, min_len=1.0), "temporal_step_moments keywords: map")
    assert rtw.temporal_moment_bytes(W, H, T) == NR.moment_elems(H, W, T) * 4
    # TemporalAccumulator(moments=True) over the hand-made frames: the chain of the witness; the default accumulator is unchanged
    dev = [(torch.from_numpy(_lib_layout(i)).to("cuda:0"), torch.from_numpy(_lib_layout(f)).to("cuda:0")) for i, f in frames]
    acc, plain = rtw.TemporalAccumulator(W, H, elem_type=T, moments=True), rtw.TemporalAccumulator(W, H, elem_type=T)
    assert acc.moment is None and plain.moment is None and not plain.moments
    with pytest.raises(ValueError, match="moments=True"):
        plain.noise_into(0x1000)
    with pytest.raises(ValueError, match="first step"):
        acc.noise_into(0x1000)
    o1, o2 = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda:0"), torch.zeros(W * H * 3, dtype=torch.float32, device="cuda:0")
    d_rho = torch.zeros(W * H, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    st = mo = cp = None
    for k in range(3):
        acc.step(cams[k], dev[k][0].data_ptr(), dev[k][1].data_ptr(), o1.data_ptr())
        plain.step(cams[k], dev[k][0].data_ptr(), dev[k][1].data_ptr(), o2.data_ptr())
        acc.noise_into(d_rho.data_ptr(), radius=1)
        torch.cuda.synchronize()
        w_out, st, mo = NR.step_moments(*frames[k], cams[k], T, st, mo, cp)
        cp = cams[k]
        _assert_same(o1.cpu().numpy().reshape(W, H, 3).transpose(1, 0, 2), w_out, f"TemporalAccumulator(moments=True), frame {k}")
        assert np.array_equal(DR.bits(o1.cpu().numpy()), DR.bits(o2.cpu().numpy())) and np.array_equal(DR.bits(acc.state.cpu().numpy()), DR.bits(plain.state.cpu().numpy()))
        _assert_same(NR.unpack_moment(acc.moment.cpu().numpy(), H, W), mo, f"TemporalAccumulator.moment, frame {k}")
        _assert_same(d_rho.cpu().numpy().reshape(W, H).T, NR.noise_map(st, mo, T, radius=1), f"TemporalAccumulator.noise_into, frame {k}")
    acc.reset()
    assert acc.moment is None and acc.frames == 0
