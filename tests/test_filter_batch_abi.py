"""Batched feature and filter passes, CPU only (include/rtw_hip.h rtw_render_features_batch_*, rtw_filter_batch_*,
rtw_render_filtered_batch_*): the 10 symbols are declared, listed and exported, the ABI version stays, the Python names exist, and every
refusal that needs no real handle is decided before any HIP call and before a handle is looked at (the dummy handles and device
pointers below are never dereferenced).  The -4 of a scene handle of the other precision needs a real handle: tests/test_gpu_filter_batch.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

BATCH_SYMBOLS = ["rtw_render_features_batch_device_f32", "rtw_render_features_batch_device_f64", "rtw_render_features_batch_f32",
                 "rtw_render_features_batch_f64", "rtw_filter_batch_device_f32", "rtw_filter_batch_device_f64", "rtw_filter_batch_f32",
                 "rtw_filter_batch_f64", "rtw_render_filtered_batch_f32", "rtw_render_filtered_batch_f64"]
# what tests/test_denoise_abi.py pins: no new C symbol carries the word
DENOIS_NAMES = ["rtw_denoise_work_bytes", "rtw_denoise_device_f32", "rtw_denoise_device_f64", "rtw_denoise_f32", "rtw_denoise_f64",
                "rtw_render_denoised_f32", "rtw_render_denoised_f64"]

BAD_DENOISE = [dict(levels=0), dict(levels=9), dict(normal_power_log2=-1), dict(normal_power_log2=8), dict(flags=2), dict(gamma=2), dict(reserved=1),
               dict(device=-2), dict(sigma_color=0.0), dict(sigma_color=float("nan")), dict(sigma_depth=-0.5), dict(sigma_depth=float("inf"))]


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="module")
def lib(rtw):
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def _d(**kw):
    from rtw_amd import _capi
    v = dict(levels=3, normal_power_log2=1, flags=1, gamma=1, device=-1, reserved=0, sigma_color=0.5, sigma_depth=0.1)
    v.update(kw)
    return _capi.Denoise(**v)


def test_batch_symbols_declared_exported_and_listed(lib, rtw):
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert len(BATCH_SYMBOLS) == len(set(BATCH_SYMBOLS)) == 10
    for name in BATCH_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
        assert "denois" not in name
    assert sorted(n for n in declared if "denois" in n) == sorted(DENOIS_NAMES)
    assert lib.rtw_abi_version() == _capi.ABI_VERSION == 4                    # additive: the ABI version stays
    assert re.search(r"#define\s+RTW_ABI_VERSION\s+4\b", header)
    for name in ("render_features_batch", "features_batch_into", "denoise_batch", "denoise_batch_into", "render_denoised_batch"):
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name
    assert callable(rtw.DeviceRenderer.features_batch_into)


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("entry", ["device", "host"])
def test_a_batched_feature_render_is_refused_without_a_device(lib, rtw, T, entry):
    """validate_batch's rules together with validate_features': nulls -> -1, n_views < 1 -> -2, the render's own checks, whole frames on one
    device, the chunk range -> -2, a batch the launch cannot number -> -5"""
    from rtw_amd import _capi
    sfx = "f64" if T is np.float64 else "f32"
    N = 3
    cams = _capi.make_cameras([rtw.t_default_cam(elem_type=T)] * N, T)
    seeds = (C.c_uint64 * N)(1, 2, 3)
    out = np.zeros(N * 96 * 54 * 8 + 4, T)
    aligned = out.ctypes.data + (-out.ctypes.data % 16)
    err = lib.rtw_last_error
    if entry == "device":
        fn = getattr(lib, "rtw_render_features_batch_device_" + sfx)
        good_scene = C.c_void_p(0x1000)                  # never dereferenced

        def call(P, begin=0, count=1, scene=good_scene, cm=cams, n=N, sd=seeds, o=aligned):
            return fn(scene, cm, n, sd, C.byref(P) if P is not None else None, begin, count, C.c_void_p(o) if o is not None else None, None)
    else:
        fn = getattr(lib, "rtw_render_features_batch_" + sfx)
        S, keep = _capi.make_scene(rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T), T)

        def call(P, begin=0, count=1, scene=S, cm=cams, n=N, sd=seeds, o=aligned):
            return fn(C.byref(scene) if scene is not None else None, cm, n, sd, C.byref(P) if P is not None else None, begin, count,
                      C.c_void_p(o) if o is not None else None)

    P = _capi.make_params(96, 54, 64)                    # 64 effective chunks
    assert call(None) == -1 and b"null" in err()
    assert call(P, scene=None) == -1 and call(P, cm=None) == -1 and call(P, o=None) == -1
    assert call(P, n=0) == -2 and b"n_views" in err()
    assert call(P, n=-1) == -2
    # the chunk range, in effective chunks
    assert call(P, begin=-1) == -2 and b"chunk range" in err()
    assert call(P, count=0) == -2 and call(P, begin=64, count=1) == -2 and call(P, begin=60, count=5) == -2
    assert call(_capi.make_params(96, 54, 20, n_chunks=8), begin=7, count=1) == -2 and b"7 chunks" in err()
    # whole frames on one device
    assert call(_capi.make_params(96, 54, 64, shard_index=0, shard_count=2)) == -2 and b"shard_count" in err()
    assert call(_capi.make_params(96, 54, 64, flags=_capi.FLAG_COMPACT_TILES)) == -2 and b"COMPACT_TILES" in err()
    assert call(_capi.make_params(96, 54, 64, flags=_capi.FLAG_RCCL_REDUCE)) == -2 and b"RCCL_REDUCE" in err()
    assert call(_capi.make_params(96, 54, 64, flags=_capi.FLAG_RAY_POOL)) == -2 and b"RAY_POOL" in err()
    assert call(_capi.make_params(96, 54, 64, devices=[0, 1])) == -2 and b"n_devices" in err()
    assert call(_capi.make_params(96, 54, 64, devices=[0])) == -2 and b"device_ids" in err()
    # the usual validation of rtw_params
    assert call(_capi.make_params(0, 54, 64)) == -2 and call(_capi.make_params(96, 0, 64)) == -2 and call(_capi.make_params(96, 54, 0)) == -2
    assert call(_capi.make_params(96, 54, 64, flags=64)) == -2 and b"unknown flags" in err()
    assert call(_capi.make_params(96, 54, 64, job_pixels=3)) == -2 and b"job_pixels" in err()
    # a batch the queues of the render, or the flat tile numbering of the feature launch, cannot hold
    assert call(P, n=2 ** 31 - 1) == -5 and b"too large" in err()
    assert call(_capi.make_params(8, 8, 1), n=2 ** 31 - 1) == -5 and b"too large" in err()
    # seeds == NULL is legal: with everything in order only the device (or, for the dummy handle, nothing we may touch) is missing
    if entry == "device":
        assert call(P, o=aligned + 4) == -2 and b"aligned" in err()
    # precedence: a bad render and a null -> the null is reported
    assert call(_capi.make_params(96, 54, 64, shard_index=0, shard_count=2), scene=None) == -1
    assert call(P, begin=-1, o=None) == -1 and call(P, n=0, cm=None) == -1
    if entry == "host" and not _has_gpu():
        assert call(P) not in (0, -1, -2, -5) and b"no HIP device" in err()
        assert call(P, sd=None) not in (0, -1, -2, -5)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_batched_device_filter_is_refused_without_a_device(lib, T):
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_filter_batch_device_" + sfx)
    W, H, N = 5, 3, 4
    n_img, n_feat, n_work = N * W * H * 3 * eb, N * W * H * 8 * eb, N * lib.rtw_denoise_work_bytes(W, H, eb)
    img, feat, out, work = 0x100000, 0x200000, 0x300000, 0x400000       # never dereferenced
    err = lib.rtw_last_error

    def call(d=None, w=W, h=H, n=N, i=img, f=feat, o=out, k=work, none=False):
        d = _d() if d is None else d
        return fn(None if none else C.byref(d), w, h, n, C.c_void_p(i), C.c_void_p(f), C.c_void_p(o), C.c_void_p(k), None)

    assert call(none=True) == -1 and b"null" in err()
    assert call(i=0) == -1 and call(f=0) == -1 and call(o=0) == -1 and call(k=0) == -1
    for bad in BAD_DENOISE:
        assert call(_d(**bad)) == -2, bad
    assert call(w=0) == -2 and call(h=0) == -2 and call(w=-5) == -2
    assert call(n=0) == -2 and b"n_views" in err()
    assert call(n=-1) == -2 and call(n=-7) == -2
    assert call(w=2 ** 31 - 1, h=2 ** 31 - 1) == -5 and b"too large" in err()
    assert call(w=1 << 15, h=1 << 15, n=1 << 10) == -5 and b"too large" in err()       # the frame is fine, the batch is not
    # alignment
    assert call(k=work + 8) == -2 and b"aligned" in err()
    assert call(f=feat + 8) == -2 and b"aligned" in err()
    assert call(i=img + 2) == -2 and call(o=out + 2) == -2
    # aliasing over the WHOLE batch's extents: the last byte of the last view, which a single frame's extent would not reach
    one_img, one_feat, one_work = n_img // N, n_feat // N, n_work // N
    assert call(o=img) == -2 and b"alias" in err()
    assert call(o=img + n_img - eb) == -2 and call(o=img - n_img + eb) == -2
    assert call(o=img + one_img) == -2 and call(o=feat + one_feat) == -2 and call(o=work + one_work) == -2
    assert call(o=feat + n_feat - eb) == -2 and call(o=work + n_work - eb) == -2 and call(o=work) == -2
    assert call(k=img) == -2 and call(k=feat + 16) == -2 and call(k=feat + n_feat - 16) == -2
    assert call(k=(img + n_img - 1) & ~15) == -2
    # precedence: a null beats a bad parameter
    assert call(_d(levels=0), o=0) == -1 and call(n=0, k=0) == -1
    if not _has_gpu():
        rc = call()                                     # everything in order: only the device is missing
        assert rc not in (0, -1, -2, -5)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_batched_host_filter_is_refused_without_a_device(lib, T):
    sfx = "f64" if T is np.float64 else "f32"
    fn = getattr(lib, "rtw_filter_batch_" + sfx)
    W, H, N = 5, 3, 4
    px = N * W * H
    buf = np.zeros(px * 16, T)
    img, feat, out = buf[:px * 3], buf[px * 3:px * 11], buf[px * 11:px * 14]
    err = lib.rtw_last_error

    def call(d=None, w=W, h=H, n=N, i=img, f=feat, o=out, none=False):
        d = _d() if d is None else d
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        return fn(None if none else C.byref(d), w, h, n, p(i), p(f), p(o))

    assert call(none=True) == -1 and b"null" in err()
    assert call(i=None) == -1 and call(f=None) == -1 and call(o=None) == -1
    for bad in BAD_DENOISE:
        assert call(_d(**bad)) == -2, bad
    assert call(w=0) == -2 and call(h=-1) == -2 and call(n=0) == -2 and call(n=-2) == -2
    assert call(w=1 << 15, h=1 << 15, n=1 << 10) == -5
    assert call(o=img) == -2 and b"alias" in err()
    assert call(o=buf[px * 3 - 1:]) == -2 and call(o=buf[px * 11 - 1:]) == -2        # the last element of the last view
    if not _has_gpu():
        assert call() not in (0, -1, -2, -5) and b"no HIP device" in err()


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_render_filtered_batch_is_refused_without_a_device(lib, rtw, T):
    """nulls, the filter's own checks, and everything a batched feature render refuses"""
    from rtw_amd import _capi
    sfx = "f64" if T is np.float64 else "f32"
    fn = getattr(lib, "rtw_render_filtered_batch_" + sfx)
    N = 3
    S, keep = _capi.make_scene(rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T), T)
    cams = _capi.make_cameras([rtw.t_default_cam(elem_type=T)] * N, T)
    out = np.zeros(N * 96 * 54 * 3, T)
    err = lib.rtw_last_error

    def call(P, d=None, scene=S, cm=cams, n=N, o=out, no_d=False):
        d = _d() if d is None else d
        return fn(C.byref(scene) if scene is not None else None, cm, n, None, C.byref(P) if P is not None else None,
                  None if no_d else C.byref(d), o.ctypes.data_as(C.c_void_p) if o is not None else None)

    P = _capi.make_params(96, 54, 4)
    assert call(None) == -1 and call(P, scene=None) == -1 and call(P, cm=None) == -1 and call(P, o=None) == -1 and call(P, no_d=True) == -1
    assert call(P, n=0) == -2 and b"n_views" in err()
    for bad in BAD_DENOISE:
        assert call(P, _d(**bad)) == -2, bad
    assert call(_capi.make_params(96, 54, 4, shard_index=0, shard_count=2)) == -2 and b"shard_count" in err()
    assert call(_capi.make_params(96, 54, 4, flags=_capi.FLAG_COMPACT_TILES)) == -2 and b"COMPACT_TILES" in err()
    assert call(_capi.make_params(96, 54, 4, flags=_capi.FLAG_RCCL_REDUCE)) == -2 and b"RCCL_REDUCE" in err()
    assert call(_capi.make_params(96, 54, 4, flags=_capi.FLAG_RAY_POOL)) == -2 and b"RAY_POOL" in err()
    assert call(_capi.make_params(96, 54, 4, devices=[0, 1])) == -2 and b"n_devices" in err()
    assert call(_capi.make_params(0, 54, 4)) == -2 and call(_capi.make_params(96, 54, 0)) == -2
    assert call(_capi.make_params(96, 54, 4, flags=64)) == -2 and b"unknown flags" in err()
    assert call(_capi.make_params(96, 54, 4, job_pixels=3)) == -2 and b"job_pixels" in err()
    assert call(P, n=2 ** 31 - 1) == -5 and b"too large" in err()
    if not _has_gpu():
        assert call(P) not in (0, -1, -2, -5) and b"no HIP device" in err()
    del keep


def test_python_validation(rtw):
    T = np.float32
    scene, cam = rtw.scene_2_spheres(elem_type=T), rtw.t_default_cam(elem_type=T)
    imgs, feats = np.zeros((2, 3, 5, 3), T), np.zeros((2, 3, 5, 8), T)
    with pytest.raises(TypeError):
        rtw.denoise_batch(imgs, feats.astype(np.float64))
    with pytest.raises(ValueError):
        rtw.denoise_batch(imgs[0], feats[0])                       # a single frame: use denoise
    with pytest.raises(ValueError):
        rtw.denoise_batch(imgs, feats[:1])
    with pytest.raises(ValueError):
        rtw.denoise_batch_into(0x1000, 0x2000, 0x3000, 0x4000, 5, 3, 2, work_bytes=rtw.denoise_work_bytes(5, 3))      # one frame's bytes for two
    with pytest.raises(ValueError):
        rtw.denoise_batch_into(0x1000, 0x2000, 0x3000, 0x4000, 5, 3, 0)
    with pytest.raises(ValueError):
        rtw.render_features_batch(scene, [], 96, 4)
    with pytest.raises(ValueError):
        rtw.render_features_batch(scene, [cam, cam], 96, 4, seeds=[1, 2, 3])
    with pytest.raises(TypeError):
        rtw.render_features_batch(scene, [cam, rtw.t_default_cam(elem_type=np.float64)], 96, 4)
    with pytest.raises(ValueError):
        rtw.render_denoised_batch(scene, [cam, cam], 96, 0)
    with pytest.raises(TypeError):
        rtw.render_denoised_batch(scene, [cam, "cam"], 96, 4)


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_the_batched_calls_fail_loudly_without_gpu(rtw):
    from rtw_amd._capi import RtwError
    T = np.float32
    scene, cam = rtw.scene_2_spheres(elem_type=T), rtw.t_default_cam(elem_type=T)
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.render_features_batch(scene, [cam, cam], 96, 4)
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.denoise_batch(np.zeros((2, 3, 5, 3), T), np.zeros((2, 3, 5, 8), T))
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.render_denoised_batch(scene, [cam, cam], 96, 4)


def test_c_batch_example_compiles_and_links(tmp_path):
    """examples/render_denoised_batch_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_denoised_batch_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "render_denoised_batch_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "4", "3"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr
