"""The temporal reprojection on the GPU (include/rtw_hip.h rtw_temporal_*, rtw_render_sequence_*) against the witness tests/temporal_ref.py.
Every comparison is on the BITS -- the image and all three planes of the state; NaN values are compared as a set.  Tolerance: NONE.
Frames (W x H): 1x1 (smallest), 5x3, 37x23 (a ragged last workgroup), 70x41 (several workgroups; taps cross workgroup and wave boundaries).
tests/test_temporal_ref.py shows that the committed seeds reach every branch of the definition on the two larger frames."""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_ref as DR
import temporal_ref as TR

pytestmark = pytest.mark.gpu

SIZES = TR.SIZES
_DEFAULT = dict(TR.DEFAULTS)


@functools.lru_cache(maxsize=None)
def _sequence(size, T):
    W, H = size
    cams, frames, state0, cam0 = TR.handmade_sequence(H, W, T, TR.SEEDS[T], 3)
    for image, feat in frames:
        image.setflags(write=False)
        feat.setflags(write=False)
    for a in state0.values():
        a.setflags(write=False)
    return cams, frames, state0, cam0


@functools.lru_cache(maxsize=None)
def _witness(size, T, first, m, demodulate, gamma):
    """step 0 of the size's sequence: a first frame, or on the hand-made previous state"""
    cams, frames, state0, cam0 = _sequence(size, T)
    return TR.step(*frames[0], cams[0], T, None if first else state0, None if first else cam0, m=m, demodulate=demodulate, gamma=gamma)


def _lib_layout(a):
    """[rows, cols, c] -> the library's memory: pixel (i, j) at j*rows + i"""
    return np.array(np.swapaxes(a, 0, 1), order="C", copy=True)


def _params(**kw):
    from rtw_amd import _capi
    v = dict(_DEFAULT)
    v.update(kw)
    return _capi.Temporal(v["m"], 1 if v["demodulate"] else 0, v["gamma"], -1, (C.c_int32 * 2)(0, 0), v["sigma_depth"], v["min_weight"], v["history_max"])


def _sfx(T):
    return "f64" if T is np.float64 else "f32"


def step_host(image, feat, cam, T, state=None, cam_prev=None, **kw):
    """rtw_temporal_* on [H, W, .] arrays and a witness-style state -> (out [H, W, 3], next state)"""
    from rtw_amd import _capi
    L = _capi.lib()
    H, W = image.shape[:2]
    img, ft = _lib_layout(image), _lib_layout(feat)
    out = np.full((W, H, 3), -7.0, T)
    nxt = np.full(TR.state_elems(H, W, T), -7.0, T)
    sp = TR.pack_state(state, T) if state is not None else None
    Cm = _capi.make_camera(cam, T)
    Cp = C.byref(_capi.make_camera(cam_prev, T)) if cam_prev is not None else None
    _capi.check(getattr(L, "rtw_temporal_" + _sfx(T))(C.byref(_params(**kw)), C.byref(Cm), Cp, W, H, img.ctypes.data_as(C.c_void_p), ft.ctypes.data_as(C.c_void_p),
                                                      sp.ctypes.data_as(C.c_void_p) if sp is not None else None, nxt.ctypes.data_as(C.c_void_p),
                                                      out.ctypes.data_as(C.c_void_p)))
    return np.swapaxes(out, 0, 1), TR.unpack_state(nxt, H, W)


class DeviceFrames:
    """the frames of a sequence and a previous state as torch tensors on cuda:0, and the device entry point on them"""

    def __init__(self, frames, T, state0=None):
        import torch
        from rtw_amd import _capi
        self.torch, self.L, self.T = torch, _capi.lib(), T
        self.H, self.W = frames[0][0].shape[:2]
        self.host = [(_lib_layout(i), _lib_layout(f)) for i, f in frames]
        self.dev = [(torch.from_numpy(i).to("cuda:0"), torch.from_numpy(f).to("cuda:0")) for i, f in self.host]
        self.n_state = TR.state_elems(self.H, self.W, T)
        assert self.n_state * np.dtype(T).itemsize == self.L.rtw_temporal_state_bytes(self.W, self.H, np.dtype(T).itemsize)
        self.host_state0 = TR.pack_state(state0, T) if state0 is not None else None
        self.state0 = torch.from_numpy(self.host_state0).to("cuda:0") if state0 is not None else None
        torch.cuda.synchronize()

    def buffers(self, poison=None):
        """-> (next state, out), filled with `poison` (default: -7)"""
        dt = self.dev[0][0].dtype
        fill = -7.0 if poison is None else poison
        return (self.torch.full((self.n_state,), fill, dtype=dt, device="cuda:0"), self.torch.full((self.W * self.H * 3,), fill, dtype=dt, device="cuda:0"))

    def run(self, k, cam, state=None, cam_prev=None, bufs=None, stream=None, **kw):
        """one step on frame k -> (next state tensor, out tensor) (not synchronised when a stream is given)"""
        from rtw_amd import _capi
        nxt, out = self.buffers() if bufs is None else bufs
        self.torch.cuda.synchronize()                              # the fills above ran on torch's stream
        Cm = _capi.make_camera(cam, self.T)
        Cp = C.byref(_capi.make_camera(cam_prev, self.T)) if cam_prev is not None else None
        img, feat = self.dev[k]
        _capi.check(getattr(self.L, "rtw_temporal_device_" + _sfx(self.T))(
            C.byref(_params(**kw)), C.byref(Cm), Cp, self.W, self.H, C.c_void_p(img.data_ptr()), C.c_void_p(feat.data_ptr()),
            C.c_void_p(state.data_ptr()) if state is not None else None, C.c_void_p(nxt.data_ptr()), C.c_void_p(out.data_ptr()),
            C.c_void_p(stream.cuda_stream) if stream is not None else None))
        if stream is None:
            self.torch.cuda.synchronize()
        return nxt, out

    def image(self, out):
        return out.cpu().numpy().reshape(self.W, self.H, 3).transpose(1, 0, 2)

    def state(self, nxt):
        return TR.unpack_state(nxt.cpu().numpy(), self.H, self.W)

    def inputs_unchanged(self):
        same = all(np.array_equal(DR.bits(t.cpu().numpy()), DR.bits(a)) for dev, host in zip(self.dev, self.host) for t, a in zip(dev, host))
        if self.state0 is not None:
            got, ref = self.state0.cpu().numpy(), self.host_state0
            same = same and np.array_equal(DR.bits(got), DR.bits(ref))
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
    """(out, state) pairs: the image and the three planes"""
    _assert_same(got[0], ref[0], what + ": image")
    nan = np.isnan(ref[0])
    assert np.array_equal(nan.any(axis=-1), nan.all(axis=-1)), f"{what}: a pixel is NaN in some channels only"
    for k in ("E", "G", "L"):
        _assert_same(got[1][k], ref[1][k], f"{what}: state plane {k}")


# ---- 1. every frame, precision and parameter set through both entry points -------------------------------------------------------------
@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_steps_equal_the_witness(T, size, entry):
    cams, frames, state0, cam0 = _sequence(size, T)
    dev = DeviceFrames(frames[:1], T, state0) if entry == "device" else None
    bufs = dev.buffers() if dev else None
    accepted = False
    for first in (True, False):
        for m in (0, 1, 7):
            for demodulate in (True, False):
                for gamma in (0, 1):
                    kw = dict(m=m, demodulate=demodulate, gamma=gamma)
                    ref = _witness(size, T, first, m, demodulate, gamma)
                    if dev:
                        nxt, out = dev.run(0, cams[0], None if first else dev.state0, None if first else cam0, bufs=bufs, **kw)
                        got = dev.image(out), dev.state(nxt)
                    else:
                        got = step_host(*frames[0], cams[0], T, None if first else state0, None if first else cam0, **kw)
                    _assert_step(got, ref, f"{np.dtype(T).name} {size} {entry} first={first} {kw}")
                    accepted = accepted or bool((ref[1]["L"] > 1).any())
    assert accepted or size[0] * size[1] < 15          # (a history was blended, not only reset)
    if dev:
        assert dev.inputs_unchanged()


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_parameters_reach_the_kernel(T):
    size = (37, 23)
    cams, frames, state0, cam0 = _sequence(size, T)
    dev = DeviceFrames(frames[:1], T, state0)
    base = _witness(size, T, False, 1, True, 1)
    for kw in (dict(sigma_depth=0.002), dict(min_weight=0.9), dict(min_weight=2.0 ** -20), dict(history_max=1.0), dict(history_max=3.5)):
        ref = TR.step(*frames[0], cams[0], T, state0, cam0, **kw)
        assert not (TR.same_bits(ref[0], base[0]) and TR.same_state(ref[1], base[1])), kw
        nxt, out = dev.run(0, cams[0], dev.state0, cam0, **kw)
        _assert_step((dev.image(out), dev.state(nxt)), ref, f"device {kw}")
        _assert_step(step_host(*frames[0], cams[0], T, state0, cam0, **kw), ref, f"host {kw}")


# ---- 2. a chain of three steps: the state of step k feeds step k + 1, all on the device --------------------------------------------------
@pytest.mark.parametrize("size", [(37, 23), (70, 41)])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_three_step_chain(T, size):
    cams, frames, state0, cam0 = _sequence(size, T)
    dev = DeviceFrames(frames, T, state0)
    for start in ("first frame", "hand-made state"):
        ref_state, ref_cam = (None, None) if start == "first frame" else (state0, cam0)
        d_state, grew = (None if start == "first frame" else dev.state0), False
        for k in range(3):
            ref_out, ref_state = TR.step(*frames[k], cams[k], T, ref_state, ref_cam)
            d_state, out = dev.run(k, cams[k], d_state, ref_cam)
            _assert_step((dev.image(out), dev.state(d_state)), (ref_out, ref_state), f"{np.dtype(T).name} {size} {start}, step {k}")
            ref_cam = cams[k]
            grew = grew or bool((ref_state["L"] > 2).any())
        assert grew                                         # (a history at least three frames long)
    assert dev.inputs_unchanged()


# ---- 3. poisoned outputs change nothing; the inputs stay; two streams --------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_poisoned_outputs_change_nothing(T):
    size = (37, 23)
    cams, frames, state0, cam0 = _sequence(size, T)
    dev = DeviceFrames(frames[:1], T, state0)
    for first in (True, False):
        for poison in (float("nan"), float("inf"), 1e30):
            nxt, out = dev.run(0, cams[0], None if first else dev.state0, None if first else cam0, bufs=dev.buffers(poison=poison))
            _assert_step((dev.image(out), dev.state(nxt)), _witness(size, T, first, 1, True, 1), f"poison {poison} first={first}")
            # the padding behind the L plane is not the kernel's to write
            assert np.array_equal(DR.bits(nxt.cpu().numpy()[9 * size[0] * size[1]:]), DR.bits(np.full(dev.n_state - 9 * size[0] * size[1], poison, T)))
    assert dev.inputs_unchanged()


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_two_streams_with_separate_states(T):
    import torch
    size = (70, 41)
    cams, frames, state0, cam0 = _sequence(size, T)
    dev = DeviceFrames(frames, T, state0)
    refs, st, cp = [], state0, cam0
    for k in range(3):
        out, st = TR.step(*frames[k], cams[k], T, st, cp)
        refs.append((out, st))
        cp = cams[k]
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    bufs = {s: [dev.buffers(poison=float("nan")) for _ in range(3)] for s in (sa, sb)}
    torch.cuda.synchronize()
    got = {sa: [], sb: []}
    state = {sa: dev.state0, sb: dev.state0}
    cp = cam0
    for k in range(3):                                     # the two chains interleaved, each ordered by its own stream
        for s in (sa, sb):
            nxt, out = dev.run(k, cams[k], state[s], cp, bufs=bufs[s][k], stream=s)
            got[s].append((nxt, out))
            state[s] = nxt
        cp = cams[k]
    sa.synchronize()
    sb.synchronize()
    for name, s in (("a", sa), ("b", sb)):
        for k in range(3):
            _assert_step((dev.image(got[s][k][1]), dev.state(got[s][k][0])), refs[k], f"stream {name}, step {k}")
    assert dev.inputs_unchanged()


# ---- 4. the sequence call equals its parts -------------------------------------------------------------------------------------------------
_STAT_KEYS = ("samples", "segments", "sphere_tests", "n_chunks", "grid_blocks", "block_threads")


def _orbit(rtw, T, n, radius=1.5, arc=0.5):
    """n pinhole cameras on an arc around the two-sphere scene's small sphere"""
    cams = []
    for v in range(n):
        phi = arc * v / max(n - 1, 1)
        cams.append(rtw.default_camera(lookfrom=(radius * np.sin(phi), 0.4, -1 + radius * np.cos(phi)), lookat=(0, 0, -1), vfov=60, aperture=0, elem_type=T))
    return cams


@pytest.mark.parametrize("denoise,group_cull", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_render_sequence_equals_its_parts(rtw, T, denoise, group_cull):
    """4 views of 32x18 at 2 spp: view v against the chain of the single calls over the product's own outputs"""
    scene, cams, seeds = rtw.scene_2_spheres(elem_type=T), _orbit(rtw, T, 4), [11, 12, 13, 14]
    tkw = dict(normal_power_log2=2, sigma_depth=0.2, min_weight=0.125, history_max=6.0)
    dkw = dict(levels=2, sigma_color=0.75)
    rtw.render_batch(scene, cams, 32, 2, seed=seeds, gamma=False, group_cull=group_cull)
    batch_stats = {k: rtw.last_stats()[k] for k in _STAT_KEYS}
    assert batch_stats["samples"] == 4 * 32 * 18 * 2
    for gamma in (True, False):
        got = rtw.render_sequence(scene, cams, 32, 2, seeds=seeds, denoise=dkw if denoise else None, gamma=gamma, group_cull=group_cull, **tkw)
        assert got.shape == (4, 18, 32, 3) and got.dtype == T and np.isfinite(got).all()
        assert {k: rtw.last_stats()[k] for k in _STAT_KEYS} == batch_stats         # rtw_stats: the render's record
        state, cam_prev, blended = None, None, False
        for v in range(4):
            lin = rtw.render(scene, cams[v], 32, 2, seed=seeds[v], gamma=False, group_cull=group_cull)
            feat = rtw.render_features(scene, cams[v], 32, 2, seed=seeds[v])["raw"]
            acc, state = rtw.temporal_step(lin, feat, cams[v], state, cam_prev, gamma=gamma and not denoise, **tkw)
            part = rtw.denoise(acc, feat, gamma=gamma, **dkw) if denoise else acc
            _assert_same(got[v], part, f"{np.dtype(T).name} view {v} denoise={denoise} gamma={gamma} cull={group_cull}")
            wit = TR.step(np.ascontiguousarray(lin), np.ascontiguousarray(feat), cams[v], T, None if v == 0 else wit[1], cam_prev, m=2, sigma_depth=0.2,
                          min_weight=0.125, history_max=6.0, gamma=int(gamma and not denoise))
            _assert_same(acc, wit[0], f"view {v}: the step against the witness")
            blended = blended or bool((wit[1]["L"] > 1).any())
            cam_prev = cams[v]
        assert blended


def test_stats_still_report_the_previous_render(rtw):
    T = np.float32
    scene, cam = rtw.scene_2_spheres(elem_type=T), rtw.t_default_cam(elem_type=T)
    rtw.render(scene, cam, 96, 4, depth=16, seed=1, device=0)
    from rtw_amd import _capi
    L = _capi.lib()
    before = _capi.Stats()
    _capi.check(L.rtw_stats(C.byref(before)))
    cams, frames, state0, cam0 = _sequence((37, 23), T)
    dev = DeviceFrames(frames[:1], T, state0)
    dev.run(0, cams[0], dev.state0, cam0)
    step_host(*frames[0], cams[0], T, state0, cam0)
    after = _capi.Stats()
    _capi.check(L.rtw_stats(C.byref(after)))
    for k, _ in _capi.Stats._fields_:
        assert getattr(before, k) == getattr(after, k), k
    assert after.samples == 96 * 54 * 4


# ---- 5. the Python layer -------------------------------------------------------------------------------------------------------------------
def test_python_layer(rtw):
    import torch
    T = np.float32
    size = (37, 23)
    cams, frames, state0, cam0 = _sequence(size, T)
    ref = _witness(size, T, False, 1, True, 1)
    from rtw_amd.features import split
    out, nxt = rtw.temporal_step(*frames[0], cams[0], TR.pack_state(state0, T), cam0)
    _assert_step((out, TR.unpack_state(nxt, 23, 37)), ref, "temporal_step")
    out, nxt = rtw.temporal_step(frames[0][0], split(frames[0][1]), cams[0], normal_power_log2=7, demodulate=False, gamma=False)
    _assert_step((out, TR.unpack_state(nxt, 23, 37)), _witness(size, T, True, 7, False, 0), "temporal_step keywords, first frame")
    assert rtw.temporal_state_bytes(37, 23, T) == TR.state_elems(23, 37, T) * 4
    # TemporalAccumulator over 3 rendered frames equals render_sequence of the same cameras and seeds
    scene, cams, seeds = rtw.scene_2_spheres(elem_type=T), _orbit(rtw, T, 3), [3, 4, 5]
    seq = rtw.render_sequence(scene, cams, 32, 2, seeds=seeds)
    acc = rtw.TemporalAccumulator(32, 18, elem_type=T)
    assert acc.state is None
    outs, dev, host = [], [], []
    for v in range(3):
        lin = rtw.render(scene, cams[v], 32, 2, seed=seeds[v], gamma=False)
        feat = rtw.render_features(scene, cams[v], 32, 2, seed=seeds[v])["raw"]
        host.append((lin, feat))
        dev.append((torch.from_numpy(_lib_layout(lin)).to("cuda:0"), torch.from_numpy(_lib_layout(feat)).to("cuda:0")))
        outs.append(torch.zeros(32 * 18 * 3, dtype=torch.float32, device="cuda:0"))
    torch.cuda.synchronize()
    for v in range(3):
        acc.step(cams[v], dev[v][0].data_ptr(), dev[v][1].data_ptr(), outs[v].data_ptr())
    torch.cuda.synchronize()
    assert acc.frames == 3 and acc.state is not None
    for v in range(3):
        _assert_same(outs[v].cpu().numpy().reshape(32, 18, 3).transpose(1, 0, 2), seq[v], f"TemporalAccumulator, frame {v}")
    firsts = [rtw.temporal_step(*host[v], cams[v])[0] for v in range(3)]
    _assert_same(seq[0], firsts[0], "view 0 is a first frame")
    assert not TR.same_bits(seq[1], firsts[1]) and not TR.same_bits(seq[2], firsts[2])          # (history was used)
    acc.reset()
    assert acc.frames == 0 and acc.state is None
    again = torch.zeros(32 * 18 * 3, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    acc.step(cams[2], dev[2][0].data_ptr(), dev[2][1].data_ptr(), again.data_ptr())
    torch.cuda.synchronize()
    _assert_same(again.cpu().numpy().reshape(32, 18, 3).transpose(1, 0, 2), firsts[2], "after reset(): a first frame")
