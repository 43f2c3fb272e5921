"""The batched render's C ABI and Python validation, CPU only (include/rtw_hip.h rtw_render_batch_*): the four symbols are declared and
exported, and every argument check the header promises is decided before any HIP call -- so these codes come back without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

BATCH_SYMBOLS = ["rtw_render_batch_f32", "rtw_render_batch_f64", "rtw_render_batch_device_f32", "rtw_render_batch_device_f64"]


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


def test_batch_symbols_declared_exported_and_listed(lib):
    import subprocess
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in BATCH_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert lib.rtw_abi_version() == 4


def _scene_and_cams(rtw, T, n):
    from rtw_amd import _capi
    flat = rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T)
    S, keep = _capi.make_scene(flat, T)
    cams = _capi.make_cameras([rtw.t_default_cam(elem_type=T)] * max(n, 1), T)
    return S, keep, cams


def _call(lib, T, S, cams, n, P, out, seeds=None):
    fn = lib.rtw_render_batch_f64 if T is np.float64 else lib.rtw_render_batch_f32
    return fn(C.byref(S) if S is not None else None, cams, n, seeds, C.byref(P), out)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_bad_arguments_are_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    S, keep, cams = _scene_and_cams(rtw, T, 2)
    out = np.empty(2 * 96 * 54 * 3, T)
    o = out.ctypes.data_as(C.c_void_p)
    P = _capi.make_params(96, 54, 4)
    assert _call(lib, T, S, cams, 0, P, o) == -2 and b"n_views" in lib.rtw_last_error()
    assert _call(lib, T, S, cams, -3, P, o) == -2
    assert _call(lib, T, S, None, 2, P, o) == -1
    assert _call(lib, T, S, cams, 2, P, None) == -1
    assert _call(lib, T, S, cams, 2, _capi.make_params(96, 54, 4, shard_index=0, shard_count=2), o) == -2
    assert b"shard_count" in lib.rtw_last_error()
    assert _call(lib, T, S, cams, 2, _capi.make_params(96, 54, 4, flags=_capi.FLAG_COMPACT_TILES), o) == -2
    assert b"COMPACT_TILES" in lib.rtw_last_error()
    assert _call(lib, T, S, cams, 2, _capi.make_params(96, 54, 4, flags=_capi.FLAG_RCCL_REDUCE), o) == -2
    assert _call(lib, T, S, cams, 2, _capi.make_params(96, 54, 4, devices=[0, 0]), o) == -2
    assert b"n_devices" in lib.rtw_last_error()
    assert _call(lib, T, S, cams, 2, _capi.make_params(96, 54, 4, devices=[0]), o) == -2          # (device_ids given)
    assert _call(lib, T, S, cams, 2, _capi.make_params(96, 54, 4, flags=_capi.FLAG_RAY_POOL), o) in (-2, -7)
    assert _call(lib, T, S, cams, 2, _capi.make_params(0, 54, 4), o) == -2                          # the single render's checks too
    # jobs beyond the 28-bit queue positions for every job shape: -5 before any allocation
    big = _capi.make_params(1 << 20, 1 << 16, 1)
    assert _call(lib, T, S, cams, 2, big, o) == -5 and b"too large" in lib.rtw_last_error()


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_device_variant_refuses_bad_arguments_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    _, _, cams = _scene_and_cams(rtw, T, 2)
    fn = lib.rtw_render_batch_device_f64 if T is np.float64 else lib.rtw_render_batch_device_f32
    P = _capi.make_params(96, 54, 4)
    dummy = C.c_void_p(0x1000)            # never dereferenced: every call below is refused before any HIP call
    assert fn(dummy, cams, 0, None, C.byref(P), dummy, None) == -2
    assert fn(dummy, None, 2, None, C.byref(P), dummy, None) == -1
    assert fn(dummy, cams, 2, None, C.byref(P), None, None) == -1
    assert fn(None, cams, 2, None, C.byref(P), dummy, None) == -1
    assert fn(dummy, cams, 2, None, C.byref(_capi.make_params(96, 54, 4, shard_index=1, shard_count=2)), dummy, None) == -2
    assert fn(dummy, cams, 2, None, C.byref(_capi.make_params(96, 54, 4, flags=_capi.FLAG_COMPACT_TILES)), dummy, None) == -2
    assert fn(dummy, cams, 2, None, C.byref(_capi.make_params(96, 54, 4, devices=[0, 1])), dummy, None) == -2


def test_render_batch_python_validation(rtw):
    scene = rtw.scene_2_spheres(elem_type=np.float32)
    cam32, cam64 = rtw.t_default_cam(elem_type=np.float32), rtw.t_default_cam(elem_type=np.float64)
    with pytest.raises(ValueError):
        rtw.render_batch(scene, [], 96, 1)
    with pytest.raises(TypeError):
        rtw.render_batch(scene, [cam32, cam64], 96, 1)
    with pytest.raises(TypeError):
        rtw.render_batch(scene, [cam32, "not a camera"], 96, 1)
    with pytest.raises(ValueError):
        rtw.render_batch(scene, [cam32, cam32, cam32], 96, 1, seed=[1, 2])
    with pytest.raises(ValueError):
        rtw.render_batch(scene, [cam32], 0, 1)
    with pytest.raises(ValueError):
        rtw.render_batch(scene, [cam32], 96, 0)
    assert "render_batch" in rtw.__all__


def test_render_batch_into_checks_the_buffer_length(rtw):
    """the length check comes before anything touches the library's device state (no device needed to see it)"""
    from rtw_amd import _capi
    T = np.float32
    dr = rtw.DeviceRenderer.__new__(rtw.DeviceRenderer)        # (no upload: the check must fire before any library call)
    dr.T, dr.L, dr.handle = T, _capi.lib(), C.c_void_p()
    cam = rtw.t_default_cam(elem_type=T)
    with pytest.raises(ValueError, match="writes"):
        dr.render_batch_into(0x1000, [cam, cam], 96, 1, n_elems=96 * 54 * 3)
    with pytest.raises(TypeError):
        dr.render_batch_into(0x1000, [rtw.t_default_cam(elem_type=np.float64)], 96, 1)


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_render_batch_fails_loudly_without_gpu(rtw):
    from rtw_amd._capi import RtwError
    scene = rtw.scene_2_spheres(elem_type=np.float32)
    cam = rtw.t_default_cam()
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.render_batch(scene, [cam, cam], 96, 1, seed=[1, 2])


def test_c_batch_example_compiles_and_links(tmp_path):
    """examples/render_batch_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    import subprocess
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_batch_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "render_batch_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "1", "3"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr and not list(tmp_path.glob("*.ppm"))
