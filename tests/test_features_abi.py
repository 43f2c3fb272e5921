"""First-hit feature buffers, CPU only (include/rtw_hip.h rtw_render_features_*): the symbols are declared, listed and exported, the ABI
version stays, and every refusal that needs no real handle is decided before any HIP call and before a handle is looked at (the dummy
handles below are never dereferenced).  The -4 of a scene handle of the other precision needs a real handle: tests/test_gpu_features.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FEATURE_SYMBOLS = ["rtw_render_features_device_f32", "rtw_render_features_device_f64", "rtw_render_features_f32", "rtw_render_features_f64"]


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


def test_feature_symbols_declared_exported_and_listed(lib, rtw):
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in FEATURE_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert lib.rtw_abi_version() == 4                    # additive: the ABI version stays
    assert re.search(r"#define\s+RTW_FEATURE_CHANNELS\s+8\b", header)
    from rtw_amd import features
    assert features.FEATURE_CHANNELS == 8
    assert "render_features" in rtw.__all__ and "features_into" in rtw.__all__
    assert callable(rtw.render_features) and callable(rtw.features_into) and callable(rtw.DeviceRenderer.features_into)


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("entry", ["device", "host"])
def test_a_feature_render_is_refused_without_a_device(lib, rtw, T, entry):
    """nulls -> -1; the render's own checks, whole frames on one device, the chunk range -> -2: all before any HIP call"""
    from rtw_amd import _capi
    sfx = "f64" if T is np.float64 else "f32"
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    out = np.zeros(96 * 54 * 8 + 4, T)
    aligned = out.ctypes.data + (-out.ctypes.data % 16)
    err = lib.rtw_last_error
    if entry == "device":
        fn = getattr(lib, "rtw_render_features_device_" + sfx)
        good_scene = C.c_void_p(0x1000)                  # never dereferenced

        def call(P, begin=0, count=1, scene=good_scene, cm=cam, o=aligned):
            return fn(scene, C.byref(cm) if cm is not None else None, C.byref(P) if P is not None else None, begin, count,
                      C.c_void_p(o) if o is not None else None, None)
    else:
        fn = getattr(lib, "rtw_render_features_" + sfx)
        S, keep = _capi.make_scene(rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T), T)

        def call(P, begin=0, count=1, scene=S, cm=cam, o=aligned):
            return fn(C.byref(scene) if scene is not None else None, C.byref(cm) if cm is not None else None,
                      C.byref(P) if P is not None else None, begin, count, C.c_void_p(o) if o is not None else None)

    P = _capi.make_params(96, 54, 64)                    # 64 effective chunks
    assert call(None) == -1 and b"null" in err()
    assert call(P, scene=None) == -1 and call(P, cm=None) == -1 and call(P, o=None) == -1
    # the chunk range, in effective chunks
    assert call(P, begin=-1) == -2 and b"chunk range" in err()
    assert call(P, count=0) == -2 and call(P, count=-3) == -2
    assert call(P, begin=64, count=1) == -2 and call(P, begin=0, count=65) == -2 and call(P, begin=60, count=5) == -2
    assert call(P, begin=2 ** 31 - 1, count=2 ** 31 - 1) == -2
    assert call(_capi.make_params(96, 54, 20, n_chunks=8), begin=7, count=1) == -2 and b"7 chunks" in err()       # s = 3: N = 7, not 8
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
    assert call(_capi.make_params(96, 54, 64, flags=_capi.FLAG_NUMERICS_CONTRACT | _capi.FLAG_NUMERICS_REFERENCE_FMA2)) == -2 and b"exclude" in err()
    assert call(_capi.make_params(96, 54, 64, job_pixels=3)) == -2 and b"job_pixels" in err()
    if entry == "device":
        assert call(P, o=aligned + 4) == -2 and b"aligned" in err()
    # precedence: a bad render and a null -> the null is reported
    assert call(_capi.make_params(96, 54, 64, shard_index=0, shard_count=2), scene=None) == -1
    assert call(P, begin=-1, o=None) == -1


def test_python_validation(rtw):
    scene = rtw.scene_2_spheres(elem_type=np.float32)
    cam = rtw.t_default_cam(elem_type=np.float32)
    with pytest.raises(ValueError):
        rtw.render_features(scene, cam, 96, 0)
    with pytest.raises(ValueError):
        rtw.render_features(scene, cam, 0, 4)
    with pytest.raises(TypeError):
        rtw.render_features(scene, cam, 96, 4, elem_type=np.int32)


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_features_fail_loudly_without_gpu(rtw):
    from rtw_amd._capi import RtwError
    scene = rtw.scene_2_spheres(elem_type=np.float32)
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.render_features(scene, rtw.t_default_cam(), 96, 4)


def test_c_features_example_compiles_and_links(tmp_path):
    """examples/render_features_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_features_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "render_features_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "8"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr
