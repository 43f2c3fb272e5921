"""The wide-aperture stage on the GPU (include/rtw_hip.h rtw_wide_aperture_*, rtw_render_wide_aperture_*) against the witness
tests/wide_aperture_ref.py.  Every comparison is on the BITS -- the image and every region of the public workspace (the narrow stage's planes,
the wide CoC and tile planes, N, the small colour, the small CoC and tile planes, O); NaN values are compared as a set.  Tolerance: NONE.
The cases are wide_aperture_ref.handmade_cases (max_radius 9, 12, 16, 17, 24 and 32, gamma 0 and 1, a focus override; their census is
asserted by tests/test_wide_aperture_ref.py) on the frames of defocus_ref.SIZES: the smallest shapes with one pixel, partial blocks, a
one-pixel last small tile (130 / 2 = 65 and 130 / 4 = 33 small pixels) and several small tiles at both scales."""
import ctypes as C
import functools

import numpy as np
import pytest

import defocus_ref as FO
import wide_aperture_ref as WA
from test_gpu_temporal_noise import _assert_same, _lib_layout, _ptr, _sfx

pytestmark = pytest.mark.gpu
PRECISIONS = [np.float32, np.float64]
GUARD = 64                          # bytes of sentinel in front of and behind the output and the workspace
SENTINEL = -7.0


@functools.lru_cache(maxsize=None)
def _cases(size, T):
    W, H = size
    cases = WA.handmade_cases(H, W, T, WA.SEEDS[T])
    for c in cases:
        c["ref"] = WA.wide_aperture(c["image"], c["features"], c["cam"], T, **c["params"])
        for a in (c["image"], c["features"], c["ref"][0], *c["ref"][1].values()):
            a.setflags(write=False)
    return cases


def _bparams(lens_radius, focus_dist=0.0, max_radius=32, gamma=0):
    from rtw_amd import _capi
    return _capi.WideAperture(max_radius, 0, gamma, -1, (C.c_int32 * 2)(0, 0), lens_radius, focus_dist)


def _device(c, T, own_stream=False, entry="rtw_wide_aperture_device_"):
    """a device entry point on one case -> (out [H, W, 3], the workspace's regions).  The output and the workspace start poisoned and sit
    between 64-byte sentinel guards that must survive; the inputs must stay"""
    import torch
    from rtw_amd import _capi
    L = _capi.lib()
    H, W = c["image"].shape[:2]
    mr = c["params"]["max_radius"]
    host = [_lib_layout(c[k]) for k in ("image", "features")]
    dev = [torch.from_numpy(a).to("cuda:0") for a in host]
    dt = torch.float64 if T is np.float64 else torch.float32
    eb = np.dtype(T).itemsize
    g = GUARD // eb
    n_work = L.rtw_wide_aperture_work_bytes(W, H, eb, mr)
    assert n_work == WA.work_elems(H, W, mr) * eb
    work = torch.full((n_work // eb + 2 * g,), SENTINEL, dtype=dt, device="cuda:0")
    out = torch.full((W * H * 3 + 2 * g,), SENTINEL, dtype=dt, device="cuda:0")
    stream = torch.cuda.Stream() if own_stream else None
    torch.cuda.synchronize()
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    b = _bparams(**c["params"])
    if entry == "rtw_defocus_device_":
        b = _capi.Defocus(b.max_radius, 0, b.gamma, -1, (C.c_int32 * 2)(0, 0), b.lens_radius, b.focus_dist)
    _capi.check(getattr(L, entry + _sfx(T))(C.byref(b), C.byref(_capi.make_camera(c["cam"], T)), W, H, vp(dev[0]), vp(dev[1]), vp(work, GUARD), vp(out, GUARD),
                                            C.c_void_p(stream.cuda_stream) if own_stream else None))
    if own_stream:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    for d, h in zip(dev, host):
        assert FO.same_bits(d.cpu().numpy(), h)
    out_h, work_h = out.cpu().numpy(), work.cpu().numpy()
    for name, a in (("output", out_h), ("workspace", work_h)):
        assert (a[:g] == SENTINEL).all() and (a[-g:] == SENTINEL).all(), f"the guards of the {name} were written"
    return out_h[g:-g].reshape(W, H, 3).transpose(1, 0, 2), WA.unpack_work(work_h[g:-g], H, W, mr)


def _host(c, T):
    from rtw_amd import _capi
    H, W = c["image"].shape[:2]
    out = np.full((W, H, 3), SENTINEL, T)
    _capi.check(getattr(_capi.lib(), "rtw_wide_aperture_" + _sfx(T))(C.byref(_bparams(**c["params"])), C.byref(_capi.make_camera(c["cam"], T)), W, H, _ptr(_lib_layout(c["image"])),
                                                                     _ptr(_lib_layout(c["features"])), _ptr(out)))
    return np.swapaxes(out, 0, 1)


@pytest.mark.parametrize("size", WA.SIZES)
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_stage_equals_the_witness(T, size):
    """every hand-made case: the device entry point's image and every region it leaves in the workspace (odd cases on a stream of the
    caller's), and the host-buffer form's image -- which thereby equals the device form's"""
    assert {c["params"]["max_radius"] for c in _cases(size, T)} >= {9, 16, 17, 32}
    for k, c in enumerate(_cases(size, T)):
        ref_out, ref_work = c["ref"]
        out, work = _device(c, T, own_stream=bool(k % 2))
        assert list(work) == list(WA.REGIONS)
        for name in WA.REGIONS:
            _assert_same(work[name], ref_work[name], f"case {k} (max_radius {c['params']['max_radius']}): the workspace's {name}")
        _assert_same(out, ref_out, f"case {k}: device")
        _assert_same(_host(c, T), ref_out, f"case {k}: host")


@pytest.mark.parametrize("T", PRECISIONS)
def test_max_radius_8_is_the_defocus_stage(T):
    """the defocus stage's own hand-made cases (max_radius 1 .. 8) through both stages' device entry points: the image and the whole
    workspace on the bits; the host-buffer form too"""
    for k, c in enumerate(FO.handmade_cases(33, 17, T, FO.SEEDS[T])[5:]):
        assert c["params"]["max_radius"] <= 8
        a_out, a_work = _device(c, T)
        b_out, b_work = _device(c, T, entry="rtw_defocus_device_")
        assert list(a_work) == ["coc", "tile"]
        _assert_same(a_out, b_out, f"case {k}: the image")
        for name in a_work:
            _assert_same(a_work[name], b_work[name], f"case {k}: the workspace's {name}")
        _assert_same(_host(c, T), b_out, f"case {k}: host")
    assert c["params"]["max_radius"] == 8


@pytest.mark.parametrize("T", PRECISIONS)
def test_a_closed_aperture_returns_the_input(T):
    """lens_radius = 0 on cases of 33 x 17 with invalid pixels: the output equals the input on the bits (NaN where not valid), gamma 0"""
    for k, c in enumerate(_cases((33, 17), T)[:6]):
        closed = dict(c, params=dict(c["params"], lens_radius=0.0, gamma=0))
        valid = ~np.isnan(c["ref"][1]["coc"][..., 1])
        for out in (_device(closed, T)[0], _host(closed, T)):
            assert FO.same_bits(out[valid], c["image"][valid]) and np.isnan(out[~valid]).all(), k


DENOISE = dict(levels=2, sigma_color=0.7)


def _cameras(rtw, T):
    """the two spheres from the side through an aperture of 1: K = 0.5 * 96 / |horizontal| is about 13 px at 96 x 54"""
    kw = dict(lookfrom=(3, 1, 2), lookat=(0, 0, -1), vup=(0, 1, 0), vfov=30, aspect_ratio=16 / 9, focus_dist=3.7, elem_type=T)
    return rtw.default_camera(aperture=1.0, **kw), rtw.default_camera(aperture=0, **kw)


@pytest.mark.parametrize("gamma", [False, True], ids=["linear", "gamma"])
@pytest.mark.parametrize("denoise", [None, DENOISE], ids=["plain", "filtered"])
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_one_call_form_is_the_chain_of_the_single_calls(rtw, T, denoise, gamma):
    """rtw_render_wide_aperture_* on scene_2_spheres through the camera with its aperture, 96 x 54 at 2 spp, with and without the filter,
    gamma 0 (max_radius 16) and 1 (max_radius 32): on the bits the render (or render + filter) and the feature pass through the pinhole
    copy with gamma 0 followed by rtw_wide_aperture_* with the gamma -- and that against the witness; lens_radius = -1 (the default of
    render_wide_aperture) is the camera's own; rtw_stats() reports the render's samples; wide_aperture_into leaves the witness's workspace"""
    import torch
    cam, pin = _cameras(rtw, T)
    scene = rtw.scene_2_spheres(elem_type=T)
    W, spp, seed, mr = 96, 2, 11, 32 if gamma else 16
    got = rtw.render_wide_aperture(scene, cam, W, spp, seed=seed, denoise=denoise, device=0, gamma=gamma, wide_aperture=dict(max_radius=mr))
    H = got.shape[0]
    st = rtw.last_stats()
    assert got.shape == (H, W, 3) == (54, 96, 3) and got.dtype == T and st["samples"] == W * H * spp
    if denoise:
        linear = rtw.render_denoised(scene, pin, W, spp, seed=seed, gamma=False, device=0, **denoise)
    else:
        linear = rtw.render(scene, pin, W, spp, seed=seed, gamma=False, device=0)
    linear = np.ascontiguousarray(linear)
    feat = np.ascontiguousarray(rtw.render_features(scene, pin, W, spp, seed=seed, device=0)["raw"])
    params = dict(lens_radius=float(cam.lens_radius), max_radius=mr)
    ref = rtw.wide_aperture(linear, feat, pin, gamma=gamma, device=0, **params)
    _assert_same(got, ref, "render_wide_aperture")
    wit_out, wit_work = WA.wide_aperture(linear, feat, pin, T, gamma=int(gamma), **params)
    assert float(wit_work["coc"][..., 0].max()) > 8 and (wit_work["lo_tile"] >= 0.5).any()
    _assert_same(ref, wit_out, "wide_aperture against the witness")
    explicit = rtw.render_wide_aperture(scene, cam, W, spp, seed=seed, denoise=denoise, device=0, gamma=gamma, wide_aperture=dict(params))
    _assert_same(explicit, got, "lens_radius = -1 against the explicit value")
    if denoise is None:
        dev = [torch.from_numpy(_lib_layout(a)).to("cuda:0") for a in (linear, feat)]
        dt = torch.float64 if T is np.float64 else torch.float32
        work = torch.zeros(rtw.wide_aperture_work_bytes(W, H, T, mr) // np.dtype(T).itemsize, dtype=dt, device="cuda:0")
        out = torch.zeros(W * H * 3, dtype=dt, device="cuda:0")
        rtw.wide_aperture_into(out.data_ptr(), work.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), pin, W, H, elem_type=T, stream=torch.cuda.current_stream().cuda_stream,
                               gamma=gamma, **params)
        torch.cuda.synchronize()
        _assert_same(out.cpu().numpy().reshape(W, H, 3).transpose(1, 0, 2), wit_out, "wide_aperture_into")
        for name, a in WA.unpack_work(work.cpu().numpy(), H, W, mr).items():
            _assert_same(a, wit_work[name], f"wide_aperture_into: the workspace's {name}")


@pytest.mark.parametrize("gamma", [False, True], ids=["linear", "gamma"])
@pytest.mark.parametrize("denoise", [None, DENOISE], ids=["plain", "filtered"])
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_one_call_forms_agree_up_to_max_radius_8(rtw, T, denoise, gamma):
    """rtw_render_defocused_* and rtw_render_wide_aperture_* with the same max_radius <= 8 return the same bits (the header: with
    max_radius <= 8 the wide-aperture call IS the defocus call): scene_2_spheres through the camera with its aperture, 96 x 54 at 2 spp,
    with and without the filter, gamma off (max_radius 5) and on (max_radius 8).  The lens is the camera's own: a point at infinity has a
    circle of K = lens_radius * W / |horizontal|, about 13 px, so both clamps bind and the frame differs from the closed aperture's."""
    cam, _ = _cameras(rtw, T)
    scene = rtw.scene_2_spheres(elem_type=T)
    W, spp, seed, mr = 96, 2, 11, 8 if gamma else 5
    assert float(cam.lens_radius) * W / float(np.linalg.norm(np.asarray(cam.horizontal, np.float64))) > 8
    kw = dict(seed=seed, denoise=denoise, device=0, gamma=gamma)
    narrow = rtw.render_defocused(scene, cam, W, spp, defocus=dict(max_radius=mr), **kw)
    wide = rtw.render_wide_aperture(scene, cam, W, spp, wide_aperture=dict(max_radius=mr), **kw)
    assert narrow.shape == wide.shape == (54, 96, 3) and narrow.dtype == wide.dtype == T
    _assert_same(wide, narrow, f"render_wide_aperture against render_defocused, max_radius {mr}")
    closed = rtw.render_defocused(scene, cam, W, spp, defocus=dict(max_radius=mr, lens_radius=0.0), **kw)
    assert not FO.same_bits(narrow, closed)
