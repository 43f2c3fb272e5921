"""The temporal clamp on the GPU (include/rtw_hip.h rtw_clamped_step_*, rtw_render_path_clamped_*) against the witness
tests/temporal_clamp_ref.py.  Every comparison is on the BITS -- the image, the three planes of the state and the moment plane; NaN values are
compared as a set.  Tolerance: NONE.
Frames (W x H; the kernel's tile is 32 rows x 8 columns): 1x1; 3x2 (smaller than the window of every radius and than a tile); 70x40 (9 x 2 tiles,
tail tiles in both directions, windows crossing tile seams); 64x36; 9x33 (exactly one tile plus one row and one column: four tiles, three of
them a single row or column wide); and the planted 12x9 step.  tests/test_temporal_clamp_ref.py shows that these inputs reach every regime of
the definition."""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_ref as DR
import temporal_clamp_ref as CR
import temporal_noise_ref as NR
import temporal_ref as TR
from test_gpu_temporal_noise import DeviceFrames, _assert_same, _lib_layout, _orbit, _ptr, _sfx, _tparams, _STAT_KEYS

pytestmark = pytest.mark.gpu

SIZES = CR.SIZES + ["planted"]
CLAMPS = [dict(radius=r, guides=g, sigma=1.0, len_scale=0.5) for r in (1, 2, 3) for g in (False, True)]
STEP_KW = [dict(m=1), dict(m=0, demodulate=False, gamma=0)]


@functools.lru_cache(maxsize=None)
def _step0(size, T):
    """-> (cam, cam_prev, (image, features), state0, moment0) of the size's step 0; read-only"""
    if size == "planted":
        cam, cp, img, feat, st, mo = CR.planted_sequence(T)
    else:
        W, H = size
        cams, frames, st, mo, cp = NR.handmade_sequence(H, W, T, CR.SEEDS[T], 1)
        cam, (img, feat) = cams[0], frames[0]
    for a in [img, feat, mo] + list(st.values()):
        a.setflags(write=False)
    return cam, cp, (img, feat), st, mo


def _key(kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def _witness(size, T, moments, ck, kw):
    cam, cp, frame, st, mo = _step0(size, T)
    return CR.step_clamped(*frame, cam, T, st, cp, mo if moments else None, clamp=dict(ck), **dict(kw))


def _cparams(**kw):
    from rtw_amd import _capi
    v = dict(CR.CLAMP_DEFAULTS)
    v.update(kw)
    return _capi.TemporalClamp(v["radius"], 1 if v["guides"] else 0, (C.c_int32 * 2)(0, 0), v["sigma"], v["len_scale"])


class ClampFrames(DeviceFrames):
    def clamped(self, k, cam, ck, state=None, moment=None, cam_prev=None, moments=True, bufs=None, **kw):
        """rtw_clamped_step_device_* on frame k -> (next state, next moments, out, an untouched buffer), synchronised"""
        from rtw_amd import _capi
        bufs = self.buffers() if bufs is None else bufs
        self.torch.cuda.synchronize()                              # the fills ran on torch's stream
        Cm, Cp = self._cams(cam, cam_prev)
        img, feat = self.dev[k]
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _capi.check(getattr(self.L, "rtw_clamped_step_device_" + _sfx(self.T))(C.byref(_tparams(**kw)), C.byref(_cparams(**ck)), C.byref(Cm), Cp, self.W, self.H, vp(img), vp(feat),
                                                                                   vp(state), vp(moment) if moments else None, vp(bufs[0]), vp(bufs[1]) if moments else None,
                                                                                   vp(bufs[2]), None))
        self.torch.cuda.synchronize()
        return bufs

    def result(self, bufs, moments=True):
        return self.image(bufs[2]), self.state(bufs[0]), (self.plane(bufs[1]) if moments else None)


def _assert_step(got, ref, what):
    _assert_same(got[0], ref[0], what + ": image")
    for k in ("E", "G", "L"):
        _assert_same(got[1][k], ref[1][k], f"{what}: state plane {k}")
    assert (got[2] is None) == (ref[2] is None), what
    if ref[2] is not None:
        _assert_same(got[2], ref[2], what + ": moment plane")


def step_host(image, feat, cam, T, ck, state=None, moment=None, cam_prev=None, moments=True, **kw):
    """rtw_clamped_step_* on [H, W, .] arrays -> (out, next state, M or None); the outputs start poisoned"""
    from rtw_amd import _capi
    L = _capi.lib()
    H, W = image.shape[:2]
    img, ft = _lib_layout(image), _lib_layout(feat)
    out = np.full((W, H, 3), -7.0, T)
    nxt, mom = np.full(TR.state_elems(H, W, T), -7.0, T), (np.full(NR.moment_elems(H, W, T), -7.0, T) if moments else None)
    sp = TR.pack_state(state, T) if state is not None else None
    mp = NR.pack_moment(moment, T) if moment is not None and moments else None
    Cm = _capi.make_camera(cam, T)
    Cp = C.byref(_capi.make_camera(cam_prev, T)) if cam_prev is not None else None
    _capi.check(getattr(L, "rtw_clamped_step_" + _sfx(T))(C.byref(_tparams(**kw)), C.byref(_cparams(**ck)), C.byref(Cm), Cp, W, H, _ptr(img), _ptr(ft), _ptr(sp), _ptr(mp), _ptr(nxt),
                                                             _ptr(mom), _ptr(out)))
    return np.swapaxes(out, 0, 1), TR.unpack_state(nxt, H, W), (NR.unpack_moment(mom, H, W) if moments else None)


# ---- 1. every frame, precision, radius, flag value, with and without moments ----------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_device_form_equals_the_witness(T, size):
    cam, cp, frame, st, mo = _step0(size, T)
    dev = ClampFrames([frame], T, st, mo)
    bufs = dev.buffers()
    for ck in CLAMPS:
        for moments in (True, False):
            for kw in STEP_KW if ck["radius"] != 2 else STEP_KW[:1]:
                ref = _witness(size, T, moments, _key(ck), _key(kw))
                dev.clamped(0, cam, ck, dev.state0, dev.moment0, cp, moments=moments, bufs=bufs, **kw)
                _assert_step(dev.result(bufs, moments), ref, f"{np.dtype(T).name} {size} {ck} moments={moments} {kw}")
    # the first frame is the plain step's
    for moments in (True, False):
        dev.clamped(0, cam, CLAMPS[0], moments=moments, bufs=bufs)
        ref = NR.step_moments(*frame, cam, T)
        _assert_step(dev.result(bufs, moments), (ref[0], ref[1], ref[2] if moments else None), f"{np.dtype(T).name} {size} first frame moments={moments}")
    assert dev.inputs_unchanged()


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_host_form_equals_the_witness(T, size):
    cam, cp, frame, st, mo = _step0(size, T)
    for ck, moments, kw in ((CLAMPS[0], True, STEP_KW[0]), (CLAMPS[5], False, STEP_KW[1]), (CLAMPS[3], True, STEP_KW[0])):
        ref = _witness(size, T, moments, _key(ck), _key(kw))
        _assert_step(step_host(*frame, cam, T, ck, st, mo, cp, moments=moments, **kw), ref, f"host {np.dtype(T).name} {size} {ck} moments={moments}")
    ref = NR.step_moments(*frame, cam, T)
    _assert_step(step_host(*frame, cam, T, CLAMPS[0]), ref, f"host {np.dtype(T).name} {size} first frame")


# ---- 2. a chain of three steps on the device --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(70, 40), (64, 36)])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_three_step_chain(T, size):
    W, H = size
    cams, frames, state0, moment0, cam0 = NR.handmade_sequence(H, W, T, CR.SEEDS[T], 3)
    dev = ClampFrames(frames, T, state0, moment0)
    ck = dict(radius=2, guides=True, sigma=1.0, len_scale=0.5)
    for start in ("first frame", "hand-made state"):
        ref = (None, None, None) if start == "first frame" else (None, state0, moment0)
        ref_cam = None if start == "first frame" else cam0
        d_st, d_mo = (None, None) if start == "first frame" else (dev.state0, dev.moment0)
        for k in range(3):
            ref = CR.step_clamped(*frames[k], cams[k], T, ref[1], ref_cam, ref[2], moments=True, clamp=ck)
            bufs = dev.clamped(k, cams[k], ck, d_st, d_mo, ref_cam)
            _assert_step(dev.result(bufs), ref, f"{np.dtype(T).name} {size} {start}, step {k}")
            d_st, d_mo, ref_cam = bufs[0], bufs[1], cams[k]
    assert dev.inputs_unchanged()


# ---- 3. poisoned outputs change nothing; nothing behind the last element is written -----------------------------------------------------------
@pytest.mark.parametrize("size", [(3, 2), (9, 33), (70, 40)])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_poisoned_outputs_change_nothing(T, size):
    cam, cp, frame, st, mo = _step0(size, T)
    dev = ClampFrames([frame], T, st, mo)
    n = dev.n
    ck = CLAMPS[3]
    ref = _witness(size, T, True, _key(ck), _key(STEP_KW[0]))
    for poison in (float("nan"), float("inf"), 1e30):
        bufs = dev.clamped(0, cam, ck, dev.state0, dev.moment0, cp, bufs=dev.buffers(poison))
        _assert_step(dev.result(bufs), ref, f"poison {poison}")
        assert np.array_equal(DR.bits(bufs[1].cpu().numpy()[n:]), DR.bits(np.full(dev.n_mom - n, poison, T)))
        assert np.array_equal(DR.bits(bufs[0].cpu().numpy()[9 * n:]), DR.bits(np.full(dev.n_state - 9 * n, poison, T)))
        assert np.array_equal(DR.bits(bufs[3].cpu().numpy()), DR.bits(np.full(dev.n_mom, poison, T)))
        # without moments the moment buffer is not the kernel's to write
        bufs = dev.clamped(0, cam, ck, dev.state0, dev.moment0, cp, moments=False, bufs=dev.buffers(poison))
        assert np.array_equal(DR.bits(bufs[1].cpu().numpy()), DR.bits(np.full(dev.n_mom, poison, T)))
    assert dev.inputs_unchanged()


# ---- 4. every parameter reaches the kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_every_parameter_reaches_the_kernel(T):
    size = (70, 40)
    cam, cp, frame, st, mo = _step0(size, T)
    dev = ClampFrames([frame], T, st, mo)
    base_k = dict(radius=1, guides=False, sigma=1.0, len_scale=1.0)
    base = _witness(size, T, True, _key(base_k), _key({}))
    _assert_step(dev.result(dev.clamped(0, cam, base_k, dev.state0, dev.moment0, cp)), base, "defaults")
    for over in (dict(radius=2), dict(radius=3), dict(guides=True), dict(sigma=0.5), dict(sigma=0.0), dict(sigma=1.5), dict(len_scale=0.5), dict(len_scale=0.0)):
        ck = dict(base_k, **over)
        ref = CR.step_clamped(*frame, cam, T, st, cp, mo, clamp=ck)
        assert not CR.same_step(ref, base), over                # (the witness says this parameter must change something here)
        _assert_step(dev.result(dev.clamped(0, cam, ck, dev.state0, dev.moment0, cp)), ref, f"device {over}")
    # the step's own parameters still reach it, the window's weights among them
    for kw in (dict(sigma_depth=0.002), dict(min_weight=0.9), dict(history_max=3.5), dict(m=3)):
        ck = dict(base_k, guides=True)
        ref = CR.step_clamped(*frame, cam, T, st, cp, mo, clamp=ck, **kw)
        assert not CR.same_step(ref, _witness(size, T, True, _key(ck), _key({}))), kw
        _assert_step(dev.result(dev.clamped(0, cam, ck, dev.state0, dev.moment0, cp, **kw)), ref, f"device {kw}")


# ---- 5. a step that moves no pixel is the plain step --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_no_movement_sequence_equals_the_plain_steps(T):
    W, H = 70, 40
    cam, cp, img, feat, st, mo = CR.no_movement_sequence(H, W, T)
    dev = ClampFrames([(img, feat)], T, st, mo)
    bits = lambda t: DR.bits(t.cpu().numpy())
    for ck in (CLAMPS[0], CLAMPS[5]):
        d = {}
        CR.step_clamped(img, feat, cam, T, st, cp, mo, clamp=ck, details=d)
        assert not d["moved"].any() and d["accept"].all()
        got = [t.clone() for t in dev.clamped(0, cam, ck, dev.state0, dev.moment0, cp)]
        ref = dev.step(0, cam, dev.state0, dev.moment0, cp)                           # rtw_history_moments_device_*
        assert all(np.array_equal(bits(got[k]), bits(ref[k])) for k in range(3)), ck
        got = [t.clone() for t in dev.clamped(0, cam, ck, dev.state0, None, cp, moments=False)]
        pn, po = dev.plain_step(0, cam, dev.state0, cp)                                # rtw_temporal_device_*
        assert np.array_equal(bits(got[0]), bits(pn)) and np.array_equal(bits(got[2]), bits(po)), ck


# ---- 6. the sequence call equals its parts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_render_path_clamped_equals_its_parts(rtw, T):
    """4 views of 96x54 at 1 spp over the two-sphere scene, in the three forms (no filter, the plain filter, the guided filter): view v against
    the chain of the single DEVICE calls over the product's own renders and features, on the bits; rtw_stats reports the render's record"""
    import torch
    W, H, N = 96, 54, 4
    scene, cams, seeds = rtw.scene_2_spheres(elem_type=T), _orbit(rtw, T, N), [31, 32, 33, 34]
    tkw = dict(normal_power_log2=1, sigma_depth=0.2, min_weight=0.125, history_max=6.0)
    nkw = dict(radius=2, normal_power_log2=1, sigma_depth=0.1, min_len=2.0)
    dkw = dict(levels=2, sigma_color=1.5)
    ck = dict(radius=2, guides=True, sigma=1.0, len_scale=0.5)
    rtw.render_batch(scene, cams, W, 1, seed=seeds, gamma=False)
    batch_stats = {k: rtw.last_stats()[k] for k in _STAT_KEYS}
    dt = torch.float64 if T is np.float64 else torch.float32
    eb = np.dtype(T).itemsize
    full = lambda k: torch.full((k,), float("nan"), dtype=dt, device="cuda:0")
    frames = []
    for v in range(N):
        lin = rtw.render(scene, cams[v], W, 1, seed=seeds[v], gamma=False)
        feat = rtw.render_features(scene, cams[v], W, 1, seed=seeds[v])["raw"]
        frames.append((torch.from_numpy(_lib_layout(lin)).to("cuda:0"), torch.from_numpy(_lib_layout(feat)).to("cuda:0")))
    plain_guided = rtw.render_sequence(scene, cams, W, 1, seeds=seeds, denoise=dkw, guided=nkw, **tkw)
    for form in ("none", "plain", "guided"):
        gamma = form != "plain"
        got = rtw.render_sequence(scene, cams, W, 1, seeds=seeds, clamp=ck, gamma=gamma, denoise=None if form == "none" else dkw, guided=nkw if form == "guided" else None, **tkw)
        assert got.shape == (N, H, W, 3) and got.dtype == T and np.isfinite(got).all()
        assert {k: rtw.last_stats()[k] for k in _STAT_KEYS} == batch_stats
        st, mo = [full(rtw.temporal_state_bytes(W, H, T) // eb) for _ in range(2)], [full(rtw.temporal_moment_bytes(W, H, T) // eb) for _ in range(2)]
        acc, rho, flt, work = full(W * H * 3), full(W * H), full(W * H * 3), torch.zeros(rtw.denoise_work_bytes(W, H, T) // eb, dtype=dt, device="cuda:0")
        cam_prev = None
        for v in range(N):
            d_lin, d_feat = frames[v]
            torch.cuda.synchronize()
            mom = form == "guided"
            rtw.temporal_step_clamped_into(acc.data_ptr(), st[v & 1].data_ptr(), d_lin.data_ptr(), d_feat.data_ptr(), cams[v], W, H, clamp=ck,
                                           d_state_prev_ptr=st[(v & 1) ^ 1].data_ptr() if v else None, d_moment_prev_ptr=mo[(v & 1) ^ 1].data_ptr() if v and mom else None,
                                           d_moment_next_ptr=mo[v & 1].data_ptr() if mom else None, cam_prev=cam_prev, elem_type=T, gamma=gamma and form == "none", **tkw)
            res = acc
            if form == "guided":
                rtw.temporal_noise_into(rho.data_ptr(), st[v & 1].data_ptr(), mo[v & 1].data_ptr(), W, H, elem_type=T, **nkw)
                rtw.denoise_guided_into(flt.data_ptr(), acc.data_ptr(), d_feat.data_ptr(), rho.data_ptr(), work.data_ptr(), W, H, elem_type=T, gamma=gamma, **dkw)
                res = flt
            elif form == "plain":
                rtw.denoise_into(flt.data_ptr(), acc.data_ptr(), d_feat.data_ptr(), work.data_ptr(), W, H, elem_type=T, gamma=gamma, **dkw)
                res = flt
            torch.cuda.synchronize()
            _assert_same(got[v], res.cpu().numpy().reshape(W, H, 3).transpose(1, 0, 2), f"{np.dtype(T).name} {form} view {v}")
            cam_prev = cams[v]
        if form == "guided":
            assert TR.same_bits(got[0], plain_guided[0]) and not TR.same_bits(got[1:], plain_guided[1:])     # (view 0 is a first frame; the clamped call is not the plain one)


# ---- 7. the Python layer ---------------------------------------------------------------------------------------------------------------------
def test_python_layer(rtw):
    import torch
    T = np.float32
    W, H = 70, 40
    cams, frames, state0, moment0, cam0 = NR.handmade_sequence(H, W, T, CR.SEEDS[T], 3)
    ck = dict(radius=2, guides=True, sigma=1.5, len_scale=0.25)
    ref = CR.step_clamped(*frames[0], cams[0], T, state0, cam0, moment0, clamp=ck)
    out, nxt, mom = rtw.temporal_step_clamped(*frames[0], cams[0], TR.pack_state(state0, T), NR.pack_moment(moment0, T), cam0, clamp=ck)
    _assert_step((out, TR.unpack_state(nxt, H, W), NR.unpack_moment(mom, H, W)), ref, "temporal_step_clamped with moments")
    out, nxt = rtw.temporal_step_clamped(*frames[0], cams[0], TR.pack_state(state0, T), cam_prev=cam0)
    ref = CR.step_clamped(*frames[0], cams[0], T, state0, cam0)
    _assert_step((out, TR.unpack_state(nxt, H, W), None), ref, "temporal_step_clamped, defaults")
    out, nxt, mom = rtw.temporal_step_clamped(*frames[0], cams[0], moments=True, normal_power_log2=0, demodulate=False, gamma=False)
    ref = NR.step_moments(*frames[0], cams[0], T, m=0, demodulate=False, gamma=0)
    _assert_step((out, TR.unpack_state(nxt, H, W), NR.unpack_moment(mom, H, W)), ref, "temporal_step_clamped, first frame")
    # TemporalAccumulator(clamp=...) over the hand-made frames: the chain of the witness, with and without moments
    dev = [(torch.from_numpy(_lib_layout(i)).to("cuda:0"), torch.from_numpy(_lib_layout(f)).to("cuda:0")) for i, f in frames]
    for moments in (True, False):
        acc = rtw.TemporalAccumulator(W, H, elem_type=T, moments=moments, clamp=ck)
        o1 = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        w, cp = (None, None, None), None
        for k in range(3):
            acc.step(cams[k], dev[k][0].data_ptr(), dev[k][1].data_ptr(), o1.data_ptr())
            torch.cuda.synchronize()
            w = CR.step_clamped(*frames[k], cams[k], T, w[1], cp, w[2], moments=moments, clamp=ck)
            cp = cams[k]
            got = (o1.cpu().numpy().reshape(W, H, 3).transpose(1, 0, 2), TR.unpack_state(acc.state.cpu().numpy(), H, W),
                   NR.unpack_moment(acc.moment.cpu().numpy(), H, W) if moments else None)
            _assert_step(got, w, f"TemporalAccumulator(clamp, moments={moments}), frame {k}")
    assert rtw.TemporalAccumulator(W, H, elem_type=T).clamp is None
