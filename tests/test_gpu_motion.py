"""Temporal reuse over moving spheres on the GPU (include/rtw_hip.h rtw_first_hit_motion_*, rtw_animated_step_*) against the witness
tests/motion_ref.py.  Every comparison is on the BITS -- the motion plane, the image, the three planes of the state and the moment plane; NaN
values are compared as a set.  Tolerance: NONE.
The pass: frame F's scene (485 spheres) at 32 x 18 through its lens camera (the lens is ignored) and a pinhole, at 1 x 1 and 5 x 3, in every
numerics mode and under the scan-mode flags; one sphere; a bubble (negative radius); two identical spheres (the lower index is named); the
scenes of tests/big_scenes.py at 16 x 9 -- 1600 / 800 spheres and both sides of the 24 KB boundary (1528 | 1529, 760 | 761), where the
instance changes from the LDS copy to scalar loads from global memory.  The step: the hand-made steps of motion_ref.handmade_steps, whose
census tests/test_motion_ref.py asserts."""
import ctypes as C
import functools

import numpy as np
import pytest

import big_scenes as BS
import features_ref as FR
import motion_ref as MR
import temporal_noise_ref as NR
import temporal_ref as TR
from conftest import NUMERICS_MODES, CamObj
from test_gpu_temporal_clamp import _cparams
from test_gpu_temporal_noise import DeviceFrames, _assert_same, _lib_layout, _ptr, _sfx, _tparams

pytestmark = pytest.mark.gpu
PRECISIONS = [np.float32, np.float64]


# ---- the motion pass ------------------------------------------------------------------------------------------------------------------------
def _small_scene(T, name):
    """hand-made scenes of a few spheres in front of a camera at (0, 0, 1) looking down -z"""
    T = np.dtype(T).type
    if name == "one":
        c, r = [(0.0, 0.0, -1.0)], [0.5]
    elif name == "bubble":                                   # a glass shell: the inner sphere has a negative radius
        c, r = [(0.0, -100.5, -1.0), (0.0, 0.0, -1.0), (0.0, 0.0, -1.0), (1.1, 0.0, -1.0)], [100.0, 0.5, -0.4, 0.5]
    else:                                                    # "twins": indices 1 and 2 are one sphere
        c, r = [(0.0, -100.5, -1.0), (0.0, 0.0, -1.0), (0.0, 0.0, -1.0), (2.0, 0.0, -1.0)], [100.0, 0.5, 0.5, 0.5]
    c = np.array(c)
    n = len(r)
    kind = np.array([0, 2, 2, 0][:n] if name == "bubble" else [0] * n, np.int32)
    return dict(n=n, cx=c[:, 0].astype(T), cy=c[:, 1].astype(T), cz=c[:, 2].astype(T), r=np.array(r, T), kind=kind, ar=np.full(n, 0.5, T), ag=np.full(n, 0.5, T),
                ab=np.full(n, 0.5, T), param=np.where(kind == 2, 1.5, 0.0).astype(T))


@functools.lru_cache(maxsize=None)
def _case(name, T):
    """-> (flat scene, camera dict, W, H)"""
    import rtw_oracle as O
    if name.startswith("F"):
        flat, cam, W, H = FR.frame_f(T)
        if name != "F lens":
            cam = O.default_camera([13, 2, 3], [0, 0, 0], [0, 1, 0], 20, 16 / 9, 0.0, 10, T)
        W, H = {"F 1x1": (1, 1), "F 5x3": (5, 3)}.get(name, (W, H))
        return flat, cam, W, H
    if name.startswith("big"):
        n = int(name.split()[1])
        return BS.scene(T, n), BS.camera_dict(BS.cameras(T)[1]), 16, 9
    return _small_scene(T, name), O.default_camera([0, 0, 1], [0, 0, -1], [0, 1, 0], 60, 16 / 9, 0.0, 2, T), 32, 18


def _table(flat, T, seed=9):
    """a motion table for a scene: random displacements, a few NaN rows"""
    n = int(flat["n"])
    rng = np.random.default_rng(seed)
    tab = np.zeros((n, 4), T)
    tab[:, 0:3] = rng.uniform(-0.5, 0.5, (n, 3)).astype(T)
    tab[rng.integers(0, n, max(1, n // 50)), 0:3] = np.nan
    tab[34 % n, 0:3] = np.nan                                # (sphere 34 of frame F's scene is in the picture)
    return tab


class Scene:
    """a flat scene uploaded to cuda:0, and the device form of the pass on it"""

    def __init__(self, flat, T):
        import torch
        from rtw_amd import _capi
        self.torch, self.L, self.T, self.n = torch, _capi.lib(), T, int(flat["n"])
        S, keep = _capi.make_scene(flat, T)
        self.handle = C.c_void_p()
        _capi.check(getattr(self.L, "rtw_scene_upload_" + _sfx(T))(C.byref(S), 0, C.byref(self.handle)))
        del keep

    def close(self):
        self.L.rtw_scene_free(self.handle)

    def motion(self, cam, W, H, table=None, flags=0, numerics=None):
        from rtw_amd import _capi
        torch = self.torch
        dt = torch.float64 if self.T is np.float64 else torch.float32
        out = torch.full((W * H * 4,), -7.0, dtype=dt, device="cuda:0")
        tab = torch.from_numpy(np.ascontiguousarray(table)).to("cuda:0") if table is not None else None
        torch.cuda.synchronize()
        P = _capi.make_params(W, H, 1, flags=flags, numerics=numerics)
        _capi.check(getattr(self.L, "rtw_first_hit_motion_device_" + _sfx(self.T))(self.handle, C.byref(_capi.make_camera(CamObj(cam), self.T)), C.byref(P),
                                                                                  C.c_void_p(tab.data_ptr()) if tab is not None else None, C.c_void_p(out.data_ptr()), None))
        torch.cuda.synchronize()
        return out.cpu().numpy().reshape(W, H, 4).transpose(1, 0, 2)


def _host_motion(flat, cam, W, H, T, table=None, numerics=None):
    from rtw_amd import _capi
    L = _capi.lib()
    S, keep = _capi.make_scene(flat, T)
    out = np.full((W, H, 4), -7.0, T)
    P = _capi.make_params(W, H, 1, numerics=numerics)
    _capi.check(getattr(L, "rtw_first_hit_motion_" + _sfx(T))(C.byref(S), C.byref(_capi.make_camera(CamObj(cam), T)), C.byref(P), _ptr(np.ascontiguousarray(table)) if table is not None else None,
                                                              _ptr(out)))
    del keep
    return np.swapaxes(out, 0, 1)


PASS_CASES = ["F lens", "F pinhole", "F 1x1", "F 5x3", "one", "bubble", "twins"]


@pytest.mark.parametrize("name", PASS_CASES)
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_pass_equals_the_witness(oracle, T, name):
    """the device form with a table and with none (zeros, the same ids), the host form, and the scan-mode flags (the same words)"""
    flat, cam, W, H = _case(name, T)
    tab = _table(flat, T)
    ref = MR.motion_pass(flat, cam, W, H, T, tab)
    sc = Scene(flat, T)
    try:
        got = sc.motion(cam, W, H, tab)
        _assert_same(got, ref, f"{name}: the motion plane")
        bare = sc.motion(cam, W, H)
        _assert_same(bare, MR.motion_pass(flat, cam, W, H, T), f"{name}: the id buffer")
        assert (bare[..., 0:3] == 0).all() and np.array_equal(bare[..., 3], ref[..., 3])
        for flags in (4, 1, 5):                              # RTW_FLAG_SCAN_VALU, RTW_FLAG_GROUP_CULL, both
            _assert_same(sc.motion(cam, W, H, tab, flags=flags), ref, f"{name}: flags {flags}")
    finally:
        sc.close()
    _assert_same(_host_motion(flat, cam, W, H, T, tab), ref, f"{name}: the host form")
    _assert_same(_host_motion(flat, cam, W, H, T), MR.motion_pass(flat, cam, W, H, T), f"{name}: the host form without a table")
    ids = ref[..., 3]
    if name == "twins":
        assert (ids == 1).any() and not (ids == 2).any()     # the lower of the two identical spheres
    if name == "bubble":
        assert (ids == 1).any() and not (ids == 2).any()     # from outside the shell hides the bubble ...
    if name in ("F lens", "F pinhole"):
        assert (ids == -1).any() and (ids == 0).any() and len(np.unique(ids)) > 20 and np.isnan(ref[..., 0]).any()


@pytest.mark.parametrize("mode", NUMERICS_MODES)
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_pass_in_every_numerics_mode(oracle, T, mode):
    flat, cam, W, H = _case("F pinhole", T)
    tab = _table(flat, T)
    with oracle.numerics(mode):
        ref = MR.motion_pass(flat, cam, W, H, T, tab)
    sc = Scene(flat, T)
    try:
        _assert_same(sc.motion(cam, W, H, tab, numerics=mode), ref, f"numerics {mode}")
    finally:
        sc.close()
    _assert_same(_host_motion(flat, cam, W, H, T, tab, numerics=mode), ref, f"numerics {mode}: the host form")


@pytest.mark.parametrize("T", PRECISIONS)
def test_the_pass_on_scenes_in_global_memory(oracle, T):
    """1600 / 800 spheres and both sides of the boundary: the LDS_SCENE = false instance (scalar loads) and the largest scene that is staged;
    every scene holds one sphere twice (big_scenes.pair_indices), so the tie rule is exercised too"""
    for n in (BS.BIG[T],) + BS.BOUNDARY[T]:
        flat, cam, W, H = _case(f"big {n}", T)
        tab = _table(flat, T)
        ref = MR.motion_pass(flat, cam, W, H, T, tab)
        first, second = BS.pair_indices(n)
        assert (ref[..., 3] == first).any() and not (ref[..., 3] == second).any(), n
        sc = Scene(flat, T)
        try:
            _assert_same(sc.motion(cam, W, H, tab), ref, f"{n} spheres")
            _assert_same(sc.motion(cam, W, H, tab, numerics="reference_fma2"), _with(oracle, "reference_fma2", flat, cam, W, H, T, tab), f"{n} spheres, reference_fma2")
        finally:
            sc.close()


def _with(oracle, mode, flat, cam, W, H, T, tab):
    with oracle.numerics(mode):
        return MR.motion_pass(flat, cam, W, H, T, tab)


# ---- the step -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _steps(size, T):
    W, H = size
    steps = MR.handmade_steps(H, W, T, MR.SEEDS[T])
    for s in steps:
        for a in [s["image"], s["features"], s["moment"], s["motion"]] + list(s["state"].values()):
            a.setflags(write=False)
    return steps


class MotionFrames(DeviceFrames):
    def animated(self, cam, ck, motion, state, moment, cam_prev, moments, **kw):
        """rtw_animated_step_device_* on frame 0 -> (out, next state, next moment plane or None) as host arrays, synchronised; the outputs start poisoned"""
        from rtw_amd import _capi
        bufs = self.buffers()
        mv = self.torch.from_numpy(_lib_layout(motion)).to("cuda:0") if motion is not None else None
        self.torch.cuda.synchronize()
        Cm, Cp = self._cams(cam, cam_prev)
        img, feat = self.dev[0]
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _capi.check(getattr(self.L, "rtw_animated_step_device_" + _sfx(self.T))(C.byref(_tparams(**kw)), C.byref(_cparams(**ck)) if ck is not None else None, C.byref(Cm), Cp, self.W,
                                                                               self.H, vp(img), vp(feat), vp(mv), vp(state), vp(bufs[0]), vp(moment) if moments else None,
                                                                               vp(bufs[1]) if moments else None, vp(bufs[2]), None))
        self.torch.cuda.synchronize()
        return self.image(bufs[2]), self.state(bufs[0]), (self.plane(bufs[1]) if moments else None)


def _host_step(s, T, ck, moments, motion, **kw):
    """rtw_animated_step_* on host arrays -> (out, next state, M or None); the outputs start poisoned"""
    from rtw_amd import _capi
    L = _capi.lib()
    H, W = s["image"].shape[:2]
    out = np.full((W, H, 3), -7.0, T)
    nxt, mom = np.full(TR.state_elems(H, W, T), -7.0, T), (np.full(NR.moment_elems(H, W, T), -7.0, T) if moments else None)
    _capi.check(getattr(L, "rtw_animated_step_" + _sfx(T))(C.byref(_tparams(**kw)), C.byref(_cparams(**ck)) if ck is not None else None, C.byref(_capi.make_camera(s["cam"], T)),
                                                           C.byref(_capi.make_camera(s["cam_prev"], T)), W, H, _ptr(_lib_layout(s["image"])), _ptr(_lib_layout(s["features"])),
                                                           _ptr(_lib_layout(motion)), _ptr(TR.pack_state(s["state"], T)), _ptr(nxt),
                                                           _ptr(NR.pack_moment(s["moment"], T)) if moments else None, _ptr(mom), _ptr(out)))
    return np.swapaxes(out, 0, 1), TR.unpack_state(nxt, H, W), (NR.unpack_moment(mom, H, W) if moments else None)


def _assert_step(got, ref, what):
    _assert_same(got[0], ref[0], what + ": image")
    for k in ("E", "G", "L"):
        _assert_same(got[1][k], ref[1][k], f"{what}: state plane {k}")
    assert (got[2] is None) == (ref[2] is None), what
    if ref[2] is not None:
        _assert_same(got[2], ref[2], what + ": moment plane")


def _ck(clamp):
    return dict(clamp, sigma=1.0, len_scale=0.5) if clamp is not None else None


@pytest.mark.parametrize("size", MR.SIZES)
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_step_equals_the_witness(T, size):
    """every hand-made step with its hand-made motion plane: plain, with moments, clamped with r = 1 and 3, with and without guides; the device
    entry on every step, the host entry on the first; one variant also with m = 0, no demodulation, linear"""
    for k, s in enumerate(_steps(size, T)):
        dev = MotionFrames([(s["image"], s["features"])], T, s["state"], s["moment"])
        for v, (moments, clamp) in enumerate(MR.VARIANTS):
            ck = _ck(clamp)
            for kw in ([dict(), dict(m=0, demodulate=False, gamma=0)] if v in (0, 3) else [dict()]):
                ref = MR.step(s["image"], s["features"], s["cam"], T, s["motion"], s["state"], s["cam_prev"], s["moment"] if moments else None, clamp=ck, **kw)
                got = dev.animated(s["cam"], ck, s["motion"], dev.state0, dev.moment0, s["cam_prev"], moments, **kw)
                _assert_step(got, ref, f"step {k} variant {v} {kw}: device")
                if k == 0:
                    _assert_step(_host_step(s, T, ck, moments, s["motion"], **kw), ref, f"step {k} variant {v} {kw}: host")
        assert dev.inputs_unchanged()


@pytest.mark.parametrize("size", [(37, 23), (9, 33), (3, 2)])
@pytest.mark.parametrize("T", PRECISIONS)
def test_zero_motion_gives_the_static_steps_words(T, size):
    """a plane of zeros (with arbitrary fourth elements): rtw_temporal_device_*, rtw_history_moments_device_* and rtw_clamped_step_device_* on the
    bits -- image, state, moments; and the first frame (no plane, no state) is the first frame of those calls"""
    from test_gpu_temporal_clamp import ClampFrames
    s = _steps(size, T)[0]
    frame = (s["image"], s["features"])
    dev, old = MotionFrames([frame], T, s["state"], s["moment"]), ClampFrames([frame], T, s["state"], s["moment"])
    zero = np.zeros_like(s["motion"])
    zero[..., 3] = s["motion"][..., 3]
    nxt, out = old.plain_step(0, s["cam"], old.state0, s["cam_prev"])
    _assert_step(dev.animated(s["cam"], None, zero, dev.state0, None, s["cam_prev"], False), (old.image(out), old.state(nxt), None), "plain")
    b = old.step(0, s["cam"], old.state0, old.moment0, s["cam_prev"])
    _assert_step(dev.animated(s["cam"], None, zero, dev.state0, dev.moment0, s["cam_prev"], True), (old.image(b[2]), old.state(b[0]), old.plane(b[1])), "moments")
    for clamp in (dict(radius=1, guides=False), dict(radius=3, guides=True)):
        ck = _ck(clamp)
        b = old.clamped(0, s["cam"], ck, old.state0, old.moment0, s["cam_prev"])
        _assert_step(dev.animated(s["cam"], ck, zero, dev.state0, dev.moment0, s["cam_prev"], True), old.result(b), f"clamped {clamp}")
    b = old.step(0, s["cam"])
    _assert_step(dev.animated(s["cam"], None, None, None, None, None, True), (old.image(b[2]), old.state(b[0]), old.plane(b[1])), "first frame")


# ---- the Python layer and the chain of calls ----------------------------------------------------------------------------------------------------
def _four_spheres(rtw, T, shift):
    """-> (a HittableList of a ground sphere and three spheres that move with `shift`, its flat form)"""
    x = np.array([0.0, 0.0, -1.2, 2.0]) + np.array([0.0, 0.11, -0.07, 0.05]) * shift
    y, r = [-100.5, 0.0, 0.0, 0.0], [100.0, 0.5, 0.5, 0.5]
    scene = rtw.HittableList([rtw.Sphere(np.array([x[k], y[k], -1.0]).astype(T), T(r[k]), rtw.Lambertian(np.array([0.5, 0.3 + 0.1 * k, 0.2]).astype(T))) for k in range(4)])
    return scene, rtw.flatten_scene(scene, T)


def _chain(rtw, scenes, cams, W, spp, seeds, clamp, denoise, T):
    """the chain of the single host-array calls, frame by frame, and with `denoise` ONE denoise_batch over what the steps left"""
    frames, feats, state = [], [], None
    for v, (scene, cam) in enumerate(zip(scenes, cams)):
        img = rtw.render(scene, cam, W, spp, seed=seeds[v], gamma=False, device=0)
        feat = rtw.render_features(scene, cam, W, spp, seed=seeds[v], device=0)["raw"]
        mv = rtw.first_hit_motion(scene, cam, W, img.shape[0], table=rtw.motion_table(scenes[v - 1], scene, T), device=0) if v else None
        out, state = rtw.temporal_step_animated(img, feat, cam, mv, state, None, cams[v - 1] if v else None, clamp=clamp, gamma=denoise is None, device=0)
        frames.append(out)
        feats.append(feat)
    frames = np.stack(frames)
    return frames if denoise is None else rtw.denoise_batch(frames, np.stack(feats), device=0, **denoise)


DENOISE = dict(levels=2, sigma_color=0.7)


@pytest.mark.parametrize("denoise", [None, DENOISE], ids=["plain", "filtered"])
@pytest.mark.parametrize("clamp", [None, dict(radius=1, guides=True, sigma=1.0, len_scale=0.5)], ids=["unclamped", "clamped"])
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_animation_call_is_the_chain_of_the_single_calls(rtw, T, clamp, denoise):
    """rtw_render_animation_*, 3 frames of a 4-sphere scene at 24 x 13, 2 spp, three of the spheres moving, with and without c and d: frame v
    equals the chain of the single calls on the bits (render, feature pass, table, motion pass, step; one batched filter pass behind
    them); with three identical scenes the call is rtw_render_sequence_* / rtw_render_path_clamped_* with the same arguments; a single
    frame is the first frame alone, and seeds=None is p->seed for every frame"""
    W, spp = 24, 2
    cams = [rtw.default_camera(lookfrom=(0.1 * v, 0.0, 1.0), lookat=(0, 0, -1), vup=(0, 1, 0), vfov=60, aspect_ratio=16 / 9, aperture=0, focus_dist=2, elem_type=T) for v in range(3)]
    scenes, _ = zip(*[_four_spheres(rtw, T, v) for v in range(3)])
    got = rtw.render_animation(scenes, cams, W, spp, seeds=[5, 6, 7], clamp=clamp, denoise=denoise, device=0)
    assert got.shape == (3, 13, W, 3) and got.dtype == T
    stats = rtw.last_stats()
    rtw.render(scenes[0], cams[0], W, spp, seed=5, gamma=False, device=0)
    assert stats["samples"] == 3 * rtw.last_stats()["samples"] > 0             # rtw_stats(): the three renders, summed
    _assert_same(got, _chain(rtw, scenes, cams, W, spp, [5, 6, 7], clamp, denoise, T), "the chain of the single calls")
    moved = _chain(rtw, scenes, cams, W, spp, [5, 6, 7], None, None, T), _chain(rtw, [scenes[0]] * 3, cams, W, spp, [5, 6, 7], None, None, T)
    assert not TR.same_bits(moved[0][2], moved[1][2])             # (the scenes do differ in the picture)
    still = rtw.render_animation([scenes[0]] * 3, cams, W, spp, seeds=[5, 6, 7], clamp=clamp, denoise=denoise, device=0)
    _assert_same(still, rtw.render_sequence(scenes[0], cams, W, spp, seeds=[5, 6, 7], clamp=clamp, denoise=denoise, device=0), "three identical scenes against render_sequence")
    one = rtw.render_animation(scenes[1:2], cams[1:2], W, spp, seed=6, clamp=clamp, denoise=denoise, device=0)
    _assert_same(one, _chain(rtw, scenes[1:2], cams[1:2], W, spp, [6], clamp, denoise, T), "one frame, seeds=None")


@pytest.mark.parametrize("clamp", [None, dict(radius=1, guides=True, sigma=1.0, len_scale=0.5)])
@pytest.mark.parametrize("T", PRECISIONS)
def test_render_animation_is_the_chain_of_the_witness(rtw, oracle, T, clamp):
    """3 frames of a 4-sphere scene at 24 x 13, 2 spp, three of the spheres moving: frame v of render_animation equals the witness's step on the
    library's own linear render and features of that frame and the witness's motion plane; with three identical scenes it equals
    render_sequence with the same arguments"""
    import rtw_oracle as O
    W, spp = 24, 2
    cams = [rtw.default_camera(lookfrom=(0.1 * v, 0.0, 1.0), lookat=(0, 0, -1), vup=(0, 1, 0), vfov=60, aspect_ratio=16 / 9, aperture=0, focus_dist=2, elem_type=T) for v in range(3)]
    scenes, flats = zip(*[_four_spheres(rtw, T, v) for v in range(3)])
    got = rtw.render_animation(scenes, cams, W, spp, seeds=[5, 6, 7], clamp=clamp, device=0)
    H = got.shape[1]
    assert got.shape == (3, H, W, 3) and got.dtype == T
    state = prev = None
    for v in range(3):
        img = rtw.render(scenes[v], cams[v], W, spp, seed=5 + v, gamma=False, device=0)
        feat = rtw.render_features(scenes[v], cams[v], W, spp, seed=5 + v, device=0)["raw"]
        mv = MR.motion_pass(flats[v], cams[v], W, H, T, MR.motion_table(flats[v - 1], flats[v], T)) if v else None
        if v:
            _assert_same(rtw.first_hit_motion(flats[v], cams[v], W, H, table=rtw.motion_table(scenes[v - 1], scenes[v], T), device=0), mv, f"frame {v}: first_hit_motion")
        out, state, _ = MR.step(np.ascontiguousarray(img), np.ascontiguousarray(feat), cams[v], T, mv, state, prev, clamp=clamp if v else None)
        prev = cams[v]
        _assert_same(got[v], out, f"frame {v}")
    still = rtw.render_animation([scenes[0]] * 3, cams, W, spp, seeds=[5, 6, 7], clamp=clamp, device=0)
    _assert_same(still, rtw.render_sequence(scenes[0], cams, W, spp, seeds=[5, 6, 7], clamp=clamp, device=0), "three identical scenes against render_sequence")
