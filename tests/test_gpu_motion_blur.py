"""The motion-blur stage on the GPU (include/rtw_hip.h rtw_velocity_blur_*, rtw_render_blurred_*) against the witness
tests/motion_blur_ref.py.  Every comparison is on the BITS -- the image, the blur plane, the tile plane and the neighbour plane of the
public workspace; NaN values are compared as a set.  Tolerance: NONE.
The cases are motion_blur_ref.handmade_blur_cases on the frames of motion_blur_ref.SIZES (below one tile, exactly one tile, a one-column
second tile, partial tiles, 5 x 3 tiles), whose census tests/test_motion_blur_ref.py asserts."""
import ctypes as C
import functools

import numpy as np
import pytest

import motion_blur_ref as BR
from test_gpu_motion import _four_spheres
from test_gpu_temporal_noise import _assert_same, _lib_layout, _ptr, _sfx, _tparams

pytestmark = pytest.mark.gpu
PRECISIONS = [np.float32, np.float64]


@functools.lru_cache(maxsize=None)
def _cases(size, T):
    W, H = size
    cases = BR.handmade_blur_cases(H, W, T, BR.SEEDS[T])
    for c in cases:
        c["ref"] = BR.blur(c["image"], c["features"], c["motion"], c["cam"], c["cam_prev"], T, **c["params"])
        for a in (c["image"], c["features"], c["motion"], c["ref"][0], *c["ref"][1].values()):
            a.setflags(write=False)
    return cases


def _bparams(taps=15, shutter=1.0, depth_extent=0.5, gamma=0):
    from rtw_amd import _capi
    return _capi.VelocityBlur(taps, 0, gamma, -1, (C.c_int32 * 2)(0, 0), shutter, depth_extent)


def _device_blur(c, T):
    """rtw_velocity_blur_device_* on one case -> (out [H, W, 3], the workspace's planes); output and workspace start poisoned; the inputs must stay"""
    import torch
    from rtw_amd import _capi
    L = _capi.lib()
    H, W = c["image"].shape[:2]
    host = [_lib_layout(c[k]) for k in ("image", "features", "motion")]
    dev = [torch.from_numpy(a).to("cuda:0") for a in host]
    dt = torch.float64 if T is np.float64 else torch.float32
    eb = np.dtype(T).itemsize
    n_work = L.rtw_velocity_blur_work_bytes(W, H, eb)
    assert n_work == BR.work_elems(H, W) * eb
    work = torch.full((n_work // eb,), -7.0, dtype=dt, device="cuda:0")
    out = torch.full((W * H * 3,), -7.0, dtype=dt, device="cuda:0")
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())
    _capi.check(getattr(L, "rtw_velocity_blur_device_" + _sfx(T))(C.byref(_bparams(**c["params"])), C.byref(_capi.make_camera(c["cam"], T)),
                                                                  C.byref(_capi.make_camera(c["cam_prev"], T)), W, H, vp(dev[0]), vp(dev[1]), vp(dev[2]), vp(work), vp(out), None))
    torch.cuda.synchronize()
    for d, h in zip(dev, host):
        assert BR.same_bits(d.cpu().numpy(), h)
    return out.cpu().numpy().reshape(W, H, 3).transpose(1, 0, 2), BR.unpack_work(work.cpu().numpy(), H, W)


def _host_blur(c, T):
    from rtw_amd import _capi
    H, W = c["image"].shape[:2]
    out = np.full((W, H, 3), -7.0, T)
    _capi.check(getattr(_capi.lib(), "rtw_velocity_blur_" + _sfx(T))(C.byref(_bparams(**c["params"])), C.byref(_capi.make_camera(c["cam"], T)), C.byref(_capi.make_camera(c["cam_prev"], T)),
                                                                     W, H, _ptr(_lib_layout(c["image"])), _ptr(_lib_layout(c["features"])), _ptr(_lib_layout(c["motion"])), _ptr(out)))
    return np.swapaxes(out, 0, 1)


@pytest.mark.parametrize("size", BR.SIZES)
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_stage_equals_the_witness(T, size):
    """every hand-made case: the device entry point's image and the three planes it leaves in the workspace, and the host-buffer form's image"""
    for k, c in enumerate(_cases(size, T)):
        ref_out, ref_work = c["ref"]
        out, work = _device_blur(c, T)
        for name in ("plane", "tile", "nb"):
            _assert_same(work[name], ref_work[name], f"case {k}: the workspace's {name}")
        _assert_same(out, ref_out, f"case {k}: device")
        _assert_same(_host_blur(c, T), ref_out, f"case {k}: host")


@pytest.mark.parametrize("T", PRECISIONS)
def test_the_python_layer(rtw, T):
    """motion_blur and motion_blur_into on one case of 37 x 23"""
    import torch
    c = _cases((37, 23), T)[1]
    H, W = c["image"].shape[:2]
    _assert_same(rtw.motion_blur(c["image"], c["features"], c["motion"], c["cam"], c["cam_prev"], **dict(c["params"], gamma=bool(c["params"]["gamma"]))), c["ref"][0], "motion_blur")
    dev = [torch.from_numpy(_lib_layout(c[k])).to("cuda:0") for k in ("image", "features", "motion")]
    dt = torch.float64 if T is np.float64 else torch.float32
    work = torch.zeros(rtw.motion_blur_work_bytes(W, H, T) // np.dtype(T).itemsize, dtype=dt, device="cuda:0")
    out = torch.zeros(W * H * 3, dtype=dt, device="cuda:0")
    rtw.motion_blur_into(out.data_ptr(), work.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), c["cam"], c["cam_prev"], W, H, elem_type=T,
                         stream=torch.cuda.current_stream().cuda_stream, **dict(c["params"], gamma=bool(c["params"]["gamma"])))
    torch.cuda.synchronize()
    _assert_same(out.cpu().numpy().reshape(W, H, 3).transpose(1, 0, 2), c["ref"][0], "motion_blur_into")


DENOISE = dict(levels=2, sigma_color=0.7)


def _animation(rtw, name, scenes, cams, W, H, spp, seeds, gamma, denoise, blur, T):
    """rtw_render_animation_* / rtw_render_blurred_* through the C ABI on a W x H frame -> img[v, i, j, :]"""
    from rtw_amd import _capi
    from rtw_amd.denoise import make_denoise
    n = len(cams)
    made = [_capi.make_scene(rtw.flatten_scene(s, T), T) for s in scenes]
    S = (type(made[0][0]) * n)(*[m[0] for m in made])
    P = _capi.make_params(W, H, spp, 16, 1, 0, 0, 1, 0, 1 if gamma else 0, 0)
    D = make_denoise(gamma=gamma, **denoise) if denoise else None
    out = np.full(n * W * H * 3, -7.0, T)
    tail = [C.byref(_bparams(**blur))] if blur is not None else []
    _capi.check(getattr(_capi.lib(), name + _sfx(T))(S, _capi.make_cameras(cams, T), n, _capi.make_seeds(seeds, n), C.byref(P), C.byref(_tparams(gamma=1 if gamma else 0)), None,
                                                     C.byref(D) if D is not None else None, *tail, _ptr(out)))
    del made
    return out.reshape(n, W, H, 3).transpose(0, 2, 1, 3)


def _features(rtw, scene, cam, W, H, spp, seed, T):
    """rtw_render_features_* over all chunks on a W x H frame -> [H, W, 8]"""
    from rtw_amd import _capi
    from rtw_amd.features import effective_chunks
    S, keep = _capi.make_scene(rtw.flatten_scene(scene, T), T)
    P = _capi.make_params(W, H, spp, 16, seed, 0, 0, 1, 0, 1, 0)
    out = np.full(W * H * 8, -7.0, T)
    _capi.check(getattr(_capi.lib(), "rtw_render_features_" + _sfx(T))(C.byref(S), C.byref(_capi.make_camera(cam, T)), C.byref(P), 0, effective_chunks(spp)[0], _ptr(out)))
    del keep
    return np.ascontiguousarray(out.reshape(W, H, 8).transpose(1, 0, 2))


@pytest.mark.parametrize("denoise", [None, DENOISE], ids=["plain", "filtered"])
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_blurred_animation_is_the_chain_of_the_single_calls(rtw, T, denoise):
    """rtw_render_blurred_*, 3 frames of 37 x 23 of a 4-sphere scene, 2 spp, three spheres and the camera moving, with and without d: frame v
    equals rtw_render_animation_* with gamma 0 followed by rtw_velocity_blur_* on frame v (its features, its motion plane, cams[v] and
    cams[v-1]) with the gamma, on the bits; frame 0 passes through with the gamma applied; render_animation(blur=...) is the same call"""
    W, H, spp, seeds = 37, 23, 2, [5, 6, 7]
    blur = dict(taps=7, shutter=1.0, depth_extent=0.5)
    cams = [rtw.default_camera(lookfrom=(0.1 * v, 0.0, 1.0), lookat=(0, 0, -1), vup=(0, 1, 0), vfov=60, aspect_ratio=W / H, aperture=0, focus_dist=2, elem_type=T) for v in range(3)]
    scenes, _ = zip(*[_four_spheres(rtw, T, 4 * v) for v in range(3)])
    got = _animation(rtw, "rtw_render_blurred_", scenes, cams, W, H, spp, seeds, True, denoise, dict(blur, gamma=0), T)      # (b->gamma is replaced by p->gamma)
    linear = _animation(rtw, "rtw_render_animation_", scenes, cams, W, H, spp, seeds, False, denoise, None, T)
    assert got.shape == linear.shape == (3, H, W, 3) and got.dtype == T
    with np.errstate(invalid="ignore"):
        _assert_same(got[0], np.sqrt(linear[0]), "frame 0 passes through")
    filtered = 0
    for v in (1, 2):
        feat = _features(rtw, scenes[v], cams[v], W, H, spp, seeds[v], T)
        mv = rtw.first_hit_motion(scenes[v], cams[v], W, H, table=rtw.motion_table(scenes[v - 1], scenes[v], T), device=0)
        ref = rtw.motion_blur(np.ascontiguousarray(linear[v]), feat, np.ascontiguousarray(mv), cams[v], cams[v - 1], gamma=True, device=0, **blur)
        _assert_same(got[v], ref, f"frame {v}")
        with np.errstate(invalid="ignore"):
            filtered += int((BR.bits(ref) != BR.bits(np.sqrt(linear[v]))).sum())
    assert filtered > 0                                  # (the blur did change pixels: the spheres do move in the picture)
    # the Python route at its own 16:9 frame: render_animation(blur=...) against the same chain
    Wp = 32
    got = rtw.render_animation(scenes, cams, Wp, spp, seeds=seeds, denoise=denoise, blur=blur, device=0)
    linear = rtw.render_animation(scenes, cams, Wp, spp, seeds=seeds, denoise=denoise, gamma=False, device=0)
    Hp = got.shape[1]
    for v in (1, 2):
        feat = rtw.render_features(scenes[v], cams[v], Wp, spp, seed=seeds[v], device=0)["raw"]
        mv = rtw.first_hit_motion(scenes[v], cams[v], Wp, Hp, table=rtw.motion_table(scenes[v - 1], scenes[v], T), device=0)
        _assert_same(got[v], rtw.motion_blur(np.ascontiguousarray(linear[v]), np.ascontiguousarray(feat), np.ascontiguousarray(mv), cams[v], cams[v - 1], gamma=True, device=0, **blur),
                     f"render_animation(blur=...): frame {v}")
    with np.errstate(invalid="ignore"):
        _assert_same(got[0], np.sqrt(linear[0]), "render_animation(blur=...): frame 0")
