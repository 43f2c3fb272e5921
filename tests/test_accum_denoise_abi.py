"""Accumulators as the denoiser's input, CPU only (include/rtw_hip.h rtw_accum_features_*, rtw_accum_noise_*, rtw_guided_filter_device_*,
rtw_accum_filtered_*): the symbols are declared, listed and exported, and every refusal that does not need a live handle is decided
before any HIP call (the dummy handles and device pointers below are never dereferenced).  The refusals that look INTO an accumulator --
its binding, its intervals, an unfinished adaptive call -- need a real one: tests/test_gpu_accum_denoise.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW_SYMBOLS = ["rtw_accum_features_f32", "rtw_accum_features_f64", "rtw_accum_noise_f32", "rtw_accum_noise_f64",
               "rtw_guided_filter_device_f32", "rtw_guided_filter_device_f64", "rtw_accum_filtered_f32", "rtw_accum_filtered_f64"]


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
    v = dict(levels=3, normal_power_log2=1, flags=1, gamma=1, device=-1, reserved=0, sigma_color=1.0, sigma_depth=0.1)
    v.update(kw)
    return _capi.Denoise(**v)


BAD_DENOISE = [dict(levels=0), dict(levels=9), dict(normal_power_log2=8), dict(flags=2), dict(flags=4), dict(gamma=2), dict(reserved=1), dict(device=-2),
               dict(sigma_color=0.0), dict(sigma_color=float("nan")), dict(sigma_depth=-0.5), dict(sigma_depth=float("inf"))]


def _bad_params(_capi, spp=64):
    return [(_capi.make_params(96, 54, spp, shard_index=0, shard_count=2), b"shard_count"), (_capi.make_params(96, 54, spp, flags=_capi.FLAG_COMPACT_TILES), b"COMPACT_TILES"),
            (_capi.make_params(96, 54, spp, flags=_capi.FLAG_RCCL_REDUCE), b"RCCL_REDUCE"), (_capi.make_params(96, 54, spp, flags=_capi.FLAG_RAY_POOL), b"RAY_POOL"),
            (_capi.make_params(96, 54, spp, devices=[0, 1]), b"n_devices"), (_capi.make_params(0, 54, spp), b"width"), (_capi.make_params(96, 54, 0), b""),
            (_capi.make_params(96, 54, spp, flags=64), b"unknown flags"), (_capi.make_params(96, 54, spp, job_pixels=3), b"job_pixels"),
            (_capi.make_params(96, 54, spp, flags=_capi.FLAG_NUMERICS_CONTRACT | _capi.FLAG_NUMERICS_REFERENCE_FMA2), b"")]


def test_symbols_declared_exported_and_listed(lib, rtw):
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert lib.rtw_abi_version() == 4                    # additive: the ABI version stays
    assert C.sizeof(_capi.Denoise) == 40                 # rtw_denoise_t is unchanged: no flag makes a call guided
    for name in ("render_adaptive_denoised", "denoise_guided_into"):
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name
    for cls, names in ((rtw.ProgressiveRenderer, ("features", "features_into", "denoised")), (rtw.AdaptiveRenderer, ("noise", "noise_into", "denoised", "features")),
                       (rtw.ProgressiveBatchRenderer, ("denoised",)), (rtw.AdaptiveBatchRenderer, ("denoised",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_feature_pass_of_an_accumulator_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    fn = lib.rtw_accum_features_f64 if T is np.float64 else lib.rtw_accum_features_f32
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    dummy, out = C.c_void_p(0x1000), 0x200000
    err = lib.rtw_last_error

    def call(P, scene=dummy, cm=cam, acc=dummy, o=out):
        return fn(scene, C.byref(cm) if cm is not None else None, C.byref(P) if P is not None else None, acc, C.c_void_p(o), None)

    P = _capi.make_params(96, 54, 64)
    assert call(None) == -1 and b"null" in err()
    assert call(P, scene=None) == -1 and call(P, cm=None) == -1 and call(P, acc=None) == -1 and call(P, o=0) == -1
    for bad, msg in _bad_params(_capi):                               # everything the device form of the feature pass refuses
        assert call(bad) == -2 and msg in err(), msg
    assert call(P, o=out + 8) == -2 and b"aligned" in err()
    assert call(_capi.make_params(2 ** 31 - 1, 2 ** 31 - 1, 4)) == -5
    assert call(_capi.make_params(96, 54, 64, shard_index=0, shard_count=2), acc=None) == -1          # a null beats a bad parameter


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_noise_map_refuses_nulls_without_a_device(lib, T):
    fn = lib.rtw_accum_noise_f64 if T is np.float64 else lib.rtw_accum_noise_f32
    assert fn(None, C.c_void_p(0x1000), None) == -1 and b"null" in lib.rtw_last_error()
    assert fn(C.c_void_p(0x1000), None, None) == -1


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_guided_device_form_is_refused_without_a_device(lib, T):
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_guided_filter_device_" + sfx)
    W, H = 5, 3
    n_img, n_feat, n_noise, n_work = W * H * 3 * eb, W * H * 8 * eb, W * H * eb, lib.rtw_denoise_work_bytes(W, H, eb)
    img, feat, out, work, noise = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000       # never dereferenced
    err = lib.rtw_last_error

    def call(d=None, w=W, h=H, i=img, f=feat, n=noise, o=out, k=work, none=False):
        d = _d() if d is None else d
        return fn(None if none else C.byref(d), w, h, C.c_void_p(i), C.c_void_p(f), C.c_void_p(n), C.c_void_p(o), C.c_void_p(k), None)

    assert call(none=True) == -1 and b"null" in err()
    assert call(i=0) == -1 and call(f=0) == -1 and call(o=0) == -1 and call(k=0) == -1
    assert call(n=0) == -1 and b"null" in err()                        # the noise pointer is what makes the call guided
    for bad in BAD_DENOISE:
        assert call(_d(**bad)) == -2, bad
    assert call(w=0) == -2 and call(h=0) == -2 and call(w=2 ** 31 - 1, h=2 ** 31 - 1) == -5
    assert call(k=work + 8) == -2 and b"aligned" in err()
    assert call(f=feat + 8) == -2 and call(i=img + 2) == -2 and call(o=out + 2) == -2
    assert call(n=noise + 2) == -2 and b"aligned" in err()
    assert call(o=img) == -2 and b"alias" in err()
    assert call(o=feat + n_feat - eb) == -2 and call(o=work + n_work - eb) == -2 and call(k=img) == -2
    assert call(o=noise) == -2 and b"alias" in err() and call(o=noise + n_noise - eb) == -2 and call(o=noise - n_img + eb) == -2
    assert call(k=noise) == -2 and b"alias" in err()
    assert call(_d(levels=0), n=0) == -1                               # a null beats a bad parameter
    if not _has_gpu():                                                 # (a call that passes every check is made only where nothing can launch)
        assert call() not in (0, -1, -2, -5)                           # everything in order: only the device is missing
        assert call(n=img) not in (0, -1, -2, -5)                      # the map may alias another INPUT: not a refusal


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_one_call_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    fn = lib.rtw_accum_filtered_f64 if T is np.float64 else lib.rtw_accum_filtered_f32
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    dummy = C.c_void_p(0x1000)
    out = np.zeros(96 * 54 * 3, T)
    err = lib.rtw_last_error

    def call(P, d=None, scene=dummy, cm=cam, acc=dummy, guided=1, o=out, no_d=False):
        d = _d() if d is None else d
        return fn(scene, C.byref(cm) if cm is not None else None, C.byref(P) if P is not None else None, None if no_d else C.byref(d), acc, guided,
                  o.ctypes.data_as(C.c_void_p) if o is not None else None)

    P = _capi.make_params(96, 54, 64)
    assert call(None) == -1 and b"null" in err()
    assert call(P, scene=None) == -1 and call(P, cm=None) == -1 and call(P, acc=None) == -1 and call(P, o=None) == -1 and call(P, no_d=True) == -1
    assert call(P, guided=2) == -2 and b"guided" in err() and call(P, guided=-1) == -2
    for bad, msg in _bad_params(_capi):
        assert call(bad) == -2 and msg in err(), msg
        assert call(bad, guided=0) == -2
    for bad in BAD_DENOISE:
        assert call(P, _d(**bad)) == -2, bad
    assert call(P, _d(levels=0), acc=None) == -1


def test_unit_op_25_validates_before_any_hip_call(lib):
    """the layout of op 25 (include/rtw_hip.h): nulls -> -1; a size or value it does not hold -> -2; 24 stays unknown"""
    out = np.zeros(64, np.float64)
    head = np.zeros(8 + 1 + 8, np.float64)

    def unit(op, count, x, y, f32=False):
        f = lib.rtw_unit_f32 if f32 else lib.rtw_unit_f64
        return f(op, count, x.ctypes.data_as(C.c_void_p) if x is not None else None, y.ctypes.data_as(C.c_void_p) if y is not None else None, None, None)

    def noise(f32=False, **kw):
        h = head.copy()
        h[:5] = [kw.get("width", 1), kw.get("height", 1), kw.get("spp", 4), kw.get("cs", 1), kw.get("floor", 0.03)]
        h[5], h[8] = kw.get("pad", 0), kw.get("chunks", 2)
        return unit(25, kw.get("count", 1), h, out, f32=f32)

    assert unit(25, 1, None, out) == -1 and unit(25, 1, head, None, f32=True) == -1
    assert unit(24, 1, head, out) == -2 and b"unknown unit op" in lib.rtw_last_error()
    assert unit(29, 1, head, out) == -2 and b"unknown unit op" in lib.rtw_last_error()      # (the first number behind the last op)
    for bad in (dict(count=0), dict(count=2), dict(width=0), dict(height=2 ** 15), dict(width=2048, height=1024), dict(spp=0), dict(cs=0), dict(cs=1.5),
                dict(floor=-1.0), dict(floor=float("nan")), dict(floor=float("inf")), dict(pad=1), dict(chunks=0), dict(chunks=1.25)):
        assert noise(**bad) == -2 and noise(f32=True, **bad) == -2, bad
    if not _has_gpu():
        for rc in (noise(), noise(f32=True)):
            assert rc > 0 or rc in (-21, -22), rc
            assert b"no HIP device" in lib.rtw_last_error()


def test_python_validation(rtw):
    with pytest.raises(ValueError):
        rtw.denoise_guided_into(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 5, 3, work_bytes=16)
    with pytest.raises(TypeError):
        rtw.render_adaptive_denoised(rtw.scene_2_spheres(elem_type=np.float32), "camera", 96, 4, tolerance=0.1)


def test_c_example_compiles_and_links(tmp_path):
    """examples/render_adaptive_denoised_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_adaptive_denoised_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "render_adaptive_denoised_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "16"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr
