"""The defocus stage on the GPU (include/rtw_hip.h rtw_defocus_*, rtw_render_defocused_*) against the witness tests/defocus_ref.py.  Every
comparison is on the BITS -- the image, the CoC plane and the tile plane of the public workspace; NaN values are compared as a set.
Tolerance: NONE.
The cases are defocus_ref.handmade_cases on the frames of defocus_ref.SIZES (one pixel, exactly one tile, 2 x 3 and 3 x 2 tiles with a
one-pixel last tile, a strip each way, 6 x 4 tiles), whose census tests/test_defocus_ref.py asserts: max_radius 1 .. 8, gamma 0 and 1, a
focus override, values planted on either side of every decision of the definition; and one rendered frame with its real features."""
import ctypes as C
import functools

import numpy as np
import pytest

import defocus_ref as FO
from test_gpu_temporal_noise import _assert_same, _lib_layout, _ptr, _sfx

pytestmark = pytest.mark.gpu
PRECISIONS = [np.float32, np.float64]
GUARD = 64                          # bytes of sentinel in front of and behind the output and the workspace
SENTINEL = -7.0


@functools.lru_cache(maxsize=None)
def _cases(size, T):
    W, H = size
    cases = FO.handmade_cases(H, W, T, FO.SEEDS[T])
    for c in cases:
        c["ref"] = FO.defocus(c["image"], c["features"], c["cam"], T, **c["params"])
        for a in (c["image"], c["features"], c["ref"][0], *c["ref"][1].values()):
            a.setflags(write=False)
    return cases


def _bparams(lens_radius, focus_dist=0.0, max_radius=8, gamma=0):
    from rtw_amd import _capi
    return _capi.Defocus(max_radius, 0, gamma, -1, (C.c_int32 * 2)(0, 0), lens_radius, focus_dist)


def _device_defocus(c, T, own_stream=False):
    """rtw_defocus_device_* on one case -> (out [H, W, 3], the workspace's planes).  The output and the workspace start poisoned and sit between
    64-byte sentinel guards that must survive; the inputs must stay"""
    import torch
    from rtw_amd import _capi
    L = _capi.lib()
    H, W = c["image"].shape[:2]
    host = [_lib_layout(c[k]) for k in ("image", "features")]
    dev = [torch.from_numpy(a).to("cuda:0") for a in host]
    dt = torch.float64 if T is np.float64 else torch.float32
    eb = np.dtype(T).itemsize
    g = GUARD // eb
    n_work = L.rtw_defocus_work_bytes(W, H, eb)
    assert n_work == FO.work_elems(H, W) * eb
    work = torch.full((n_work // eb + 2 * g,), SENTINEL, dtype=dt, device="cuda:0")
    out = torch.full((W * H * 3 + 2 * g,), SENTINEL, dtype=dt, device="cuda:0")
    stream = torch.cuda.Stream() if own_stream else None
    torch.cuda.synchronize()
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    _capi.check(getattr(L, "rtw_defocus_device_" + _sfx(T))(C.byref(_bparams(**c["params"])), C.byref(_capi.make_camera(c["cam"], T)), W, H, vp(dev[0]), vp(dev[1]), vp(work, GUARD),
                                                            vp(out, GUARD), C.c_void_p(stream.cuda_stream) if own_stream else None))
    if own_stream:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    for d, h in zip(dev, host):
        assert FO.same_bits(d.cpu().numpy(), h)
    out_h, work_h = out.cpu().numpy(), work.cpu().numpy()
    for name, a in (("output", out_h), ("workspace", work_h)):
        assert (a[:g] == SENTINEL).all() and (a[-g:] == SENTINEL).all(), f"the guards of the {name} were written"
    return out_h[g:-g].reshape(W, H, 3).transpose(1, 0, 2), FO.unpack_work(work_h[g:-g], H, W)


def _host_defocus(c, T):
    from rtw_amd import _capi
    H, W = c["image"].shape[:2]
    out = np.full((W, H, 3), SENTINEL, T)
    _capi.check(getattr(_capi.lib(), "rtw_defocus_" + _sfx(T))(C.byref(_bparams(**c["params"])), C.byref(_capi.make_camera(c["cam"], T)), W, H, _ptr(_lib_layout(c["image"])),
                                                               _ptr(_lib_layout(c["features"])), _ptr(out)))
    return np.swapaxes(out, 0, 1)


@pytest.mark.parametrize("size", FO.SIZES)
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_stage_equals_the_witness(T, size):
    """every hand-made case: the device entry point's image and the two planes it leaves in the workspace (odd cases on a stream of the
    caller's), and the host-buffer form's image"""
    for k, c in enumerate(_cases(size, T)):
        ref_out, ref_work = c["ref"]
        out, work = _device_defocus(c, T, own_stream=bool(k % 2))
        for name in ("coc", "tile"):
            _assert_same(work[name], ref_work[name], f"case {k}: the workspace's {name}")
        _assert_same(out, ref_out, f"case {k}: device")
        _assert_same(_host_defocus(c, T), ref_out, f"case {k}: host")


@pytest.mark.parametrize("T", PRECISIONS)
def test_a_closed_aperture_returns_the_input(T):
    """lens_radius = 0 on the cases of 33 x 17 with invalid pixels: the output equals the input on the bits (NaN where not valid), gamma 0"""
    for k, c in enumerate(_cases((33, 17), T)[3:8]):
        closed = dict(c, params=dict(c["params"], lens_radius=0.0, gamma=0))
        valid = ~np.isnan(c["ref"][1]["coc"][..., 1])
        for out in (_device_defocus(closed, T)[0], _host_defocus(closed, T)):
            assert FO.same_bits(out[valid], c["image"][valid]) and np.isnan(out[~valid]).all(), k


DENOISE = dict(levels=2, sigma_color=0.7)


def _cameras(rtw, T):
    kw = dict(lookfrom=(13, 2, 3), lookat=(0, 0, 0), vup=(0, 1, 0), vfov=20, aspect_ratio=16 / 9, focus_dist=10, elem_type=T)
    return rtw.default_camera(aperture=0.6, **kw), rtw.default_camera(aperture=0, **kw)


@pytest.mark.parametrize("T", PRECISIONS)
def test_a_rendered_frame_and_the_python_layer(rtw, T):
    """scene_random_spheres through the prototype's camera, 96 x 54 at 4 spp, rendered through the pinhole with its real features: defocus and
    defocus_into against the witness"""
    import torch
    cam, pin = _cameras(rtw, T)
    scene = rtw.scene_random_spheres(elem_type=T)
    W, spp = 96, 4
    linear = np.ascontiguousarray(rtw.render(scene, pin, W, spp, seed=3, gamma=False, device=0))
    feat = np.ascontiguousarray(rtw.render_features(scene, pin, W, spp, seed=3, device=0)["raw"])
    H = linear.shape[0]
    params = dict(lens_radius=float(cam.lens_radius), focus_dist=0.0, max_radius=8)
    ref_out, ref_work = FO.defocus(linear, feat, pin, T, gamma=1, **params)
    assert (ref_work["tile"] >= 0.5).any() and float(ref_work["coc"][..., 0].max()) > 3
    _assert_same(rtw.defocus(linear, feat, pin, gamma=True, device=0, **params), ref_out, "defocus")
    dev = [torch.from_numpy(_lib_layout(a)).to("cuda:0") for a in (linear, feat)]
    dt = torch.float64 if T is np.float64 else torch.float32
    work = torch.zeros(rtw.defocus_work_bytes(W, H, T) // np.dtype(T).itemsize, dtype=dt, device="cuda:0")
    out = torch.zeros(W * H * 3, dtype=dt, device="cuda:0")
    rtw.defocus_into(out.data_ptr(), work.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), pin, W, H, elem_type=T, stream=torch.cuda.current_stream().cuda_stream, gamma=True, **params)
    torch.cuda.synchronize()
    _assert_same(out.cpu().numpy().reshape(W, H, 3).transpose(1, 0, 2), ref_out, "defocus_into")
    got = FO.unpack_work(work.cpu().numpy(), H, W)
    for name in ("coc", "tile"):
        _assert_same(got[name], ref_work[name], f"defocus_into: the workspace's {name}")


@pytest.mark.parametrize("denoise", [None, DENOISE], ids=["plain", "filtered"])
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_one_call_form_is_the_chain_of_the_single_calls(rtw, T, denoise):
    """rtw_render_defocused_* through the camera with its aperture, 64 x 36 at 2 spp, with and without the filter: on the bits the render (or
    render + filter) and the feature pass through the pinhole copy with gamma 0 followed by rtw_defocus_* with the gamma; lens_radius = -1
    (the default of render_defocused) is the camera's own; rtw_stats() reports the render's samples"""
    cam, pin = _cameras(rtw, T)
    scene = rtw.scene_random_spheres(elem_type=T)
    W, spp, seed = 64, 2, 11
    got = rtw.render_defocused(scene, cam, W, spp, seed=seed, denoise=denoise, device=0)
    H = got.shape[0]
    st = rtw.last_stats()
    assert got.shape == (H, W, 3) and got.dtype == T and st["samples"] == W * H * spp
    if denoise:
        linear = rtw.render_denoised(scene, pin, W, spp, seed=seed, gamma=False, device=0, **denoise)
    else:
        linear = rtw.render(scene, pin, W, spp, seed=seed, gamma=False, device=0)
    feat = rtw.render_features(scene, pin, W, spp, seed=seed, device=0)["raw"]
    ref = rtw.defocus(np.ascontiguousarray(linear), np.ascontiguousarray(feat), pin, lens_radius=float(cam.lens_radius), gamma=True, device=0)
    _assert_same(got, ref, "render_defocused")
    with np.errstate(invalid="ignore"):
        assert (FO.bits(ref) != FO.bits(np.sqrt(linear))).mean() > 0.5             # (the stage did change the picture)
    explicit = rtw.render_defocused(scene, cam, W, spp, seed=seed, denoise=denoise, device=0, defocus=dict(lens_radius=float(cam.lens_radius)))
    _assert_same(explicit, got, "lens_radius = -1 against the explicit value")
    rack = rtw.render_defocused(scene, cam, W, spp, seed=seed, denoise=denoise, device=0, defocus=dict(focus_dist=13.0, max_radius=3), gamma=False)
    _assert_same(rack, rtw.defocus(np.ascontiguousarray(linear), np.ascontiguousarray(feat), pin, lens_radius=float(cam.lens_radius), focus_dist=13.0, max_radius=3, gamma=False,
                                   device=0), "a focus override and max_radius 3, linear")
