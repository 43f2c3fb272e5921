"""The present stage, CPU only (include/rtw_hip.h rtw_present_*): the eleven names are declared, listed and exported, the struct has its 32
bytes, and every refusal is decided before any HIP call (the dummy device pointers below are never dereferenced)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PRESENT_SYMBOLS = ["rtw_present_bytes", "rtw_present_device_f32", "rtw_present_device_f64", "rtw_present_batch_device_f32", "rtw_present_batch_device_f64",
                   "rtw_present_f32", "rtw_present_f64", "rtw_render_presented_f32", "rtw_render_presented_f64", "rtw_render_presented_batch_f32",
                   "rtw_render_presented_batch_f64"]


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


def _p(**kw):
    from rtw_amd import _capi
    v = dict(channels=3, flags=0, device=-1, nan_rgb=(C.c_uint8 * 3)(0, 0, 0), reserved0=0, exposure=1.0, reserved=(C.c_int32 * 2)(0, 0))
    v.update(kw)
    return _capi.Present(**v)


BAD_PARAMS = [dict(channels=0), dict(channels=2), dict(channels=5), dict(channels=-3), dict(flags=8), dict(flags=16), dict(flags=-1), dict(reserved0=1),
              dict(reserved=(C.c_int32 * 2)(1, 0)), dict(reserved=(C.c_int32 * 2)(0, 1)), dict(device=-2), dict(exposure=0.0), dict(exposure=-1.0),
              dict(exposure=float("inf")), dict(exposure=float("nan"))]


def test_present_symbols_declared_exported_and_listed(lib, rtw):
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert len(PRESENT_SYMBOLS) == 11
    for name in PRESENT_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert sorted(n for n in declared if "present" in n) == sorted(PRESENT_SYMBOLS)
    assert lib.rtw_abi_version() == _capi.ABI_VERSION == 4                    # additive: the ABI version stays
    for flag, value in (("DITHER", 1), ("BGR", 2), ("SQRT", 4)):
        assert re.search(r"#define\s+RTW_PRESENT_%s\s+%d\b" % (flag, value), header) and getattr(_capi, "PRESENT_" + flag) == value
    assert "imageio.to_u8" in header                                         # what ties the stage to the 8-bit image the project defines
    for name in ("make_present", "present_bytes", "present", "present_into", "present_batch_into", "render_presented", "render_presented_batch"):
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name


def test_the_struct_has_32_bytes(tmp_path):
    from rtw_amd import _capi
    P = _capi.Present
    assert C.sizeof(P) == 32
    offs = [getattr(P, k).offset for k in ("channels", "flags", "device", "nan_rgb", "reserved0", "exposure", "reserved")]
    assert offs == [0, 4, 8, 12, 15, 16, 24]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtw_hip.h"\n'
                   '#define O(f) (int)offsetof(rtw_present_t, f)\n'
                   'int main(void) { printf("%d %d %d %d %d %d %d %d\\n", (int)sizeof(rtw_present_t), O(channels), O(flags), O(device), O(nan_rgb), O(reserved0), '
                   'O(exposure), O(reserved)); return 0; }\n')
    exe = str(tmp_path / "size")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()] == [32] + offs


def test_present_bytes(lib):
    pb, err = lib.rtw_present_bytes, lib.rtw_last_error
    assert pb(96, 54, 3, 0) == 96 * 54 * 3 == pb(96, 54, 3, 1) and pb(96, 54, 4, 0) == 96 * 54 * 4
    assert pb(67, 35, 3, 3) == 3 * 67 * 35 * 3 and pb(1, 1, 3, 0) == 3
    assert pb(1 << 16, 1 << 16, 4, 8) == 1 << 37                               # 64-bit: not truncated
    assert pb(96, 54, 2, 0) == -2 and b"channels" in err() and pb(96, 54, 5, 0) == -2 and pb(96, 54, 0, 0) == -2
    assert pb(0, 54, 3, 0) == -2 and pb(96, 0, 3, 0) == -2 and pb(-1, 54, 3, 0) == -2
    assert pb(96, 54, 3, -1) == -2 and b"n_views" in err()
    assert pb(2 ** 31 - 1, 2 ** 31 - 1, 3, 0) == -5 and b"too large" in err()
    assert pb(1 << 17, 1 << 17, 3, 512) == -5 and pb(1 << 17, 1 << 17, 3, 511) > 0          # 2^31 tiles of 64 x 64 over all views


@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_device_forms_are_refused_without_a_device(lib, T, batch):
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, ("rtw_present_batch_device_" if batch else "rtw_present_device_") + sfx)
    W, H, N = 5, 3, 2 if batch else 1
    img, out = 0x100000, 0x200000                                           # never dereferenced
    n_img = W * H * 3 * eb * N
    err = lib.rtw_last_error

    def call(p=None, w=W, h=H, n=N, i=img, o=out, none=False):
        p = _p() if p is None else p
        views = (n,) if batch else ()
        return fn(None if none else C.byref(p), w, h, *views, C.c_void_p(i), C.c_void_p(o), None)

    assert call(none=True) == -1 and b"null" in err()
    assert call(i=0) == -1 and call(o=0) == -1
    for bad in BAD_PARAMS:
        assert call(_p(**bad)) == -2 and err(), bad
    assert call(_p(flags=8)) == -2 and b"flags" in err() and call(_p(exposure=0.0)) == -2 and b"exposure" in err()
    assert call(_p(channels=2)) == -2 and b"channels" in err() and call(_p(reserved0=1)) == -2 and b"reserved" in err()
    assert call(w=0) == -2 and call(h=0) == -2 and call(w=-5) == -2
    if batch:
        assert call(n=0) == -2 and call(n=-1) == -2 and b"n_views" in err()
        assert call(w=1 << 17, h=1 << 17, n=512) == -5 and b"too large" in err()
    assert call(w=2 ** 31 - 1, h=2 ** 31 - 1) == -5 and b"too large" in err()
    # alignment: the output to 4 bytes, the input to its element type
    assert call(o=out + 1) == -2 and b"aligned" in err() and call(o=out + 2) == -2
    assert call(i=img + 2) == -2 and b"aligned" in err()
    if eb == 8:
        assert call(i=img + 4) == -2
    # overlap: the output over the input's first and last bytes, and its own last bytes over the input's first
    for ch in (3, 4):
        n_out = W * H * ch * N
        p = _p(channels=ch)
        assert call(p, o=img) == -2 and b"alias" in err()
        assert call(p, o=img + n_img - 4) == -2 and call(p, o=img - (n_out - 1) // 4 * 4) == -2
    # precedence: a null beats a bad parameter
    assert call(_p(channels=7), o=0) == -1
    if not _has_gpu():                                                       # (with a device these dummy pointers must never reach a launch)
        assert call() not in (0, -1, -2, -5)                                 # everything in order: only the device is missing
        assert call(o=img + n_img) == call() and call(_p(channels=4), o=img - W * H * 4 * N) == call()     # touching is not overlapping


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_host_form_is_refused_without_a_device(lib, T):
    fn = getattr(lib, "rtw_present_" + ("f64" if T is np.float64 else "f32"))
    W, H = 5, 3
    img = np.zeros(W * H * 3, T)
    out = np.zeros(W * H * 4, np.uint8)
    err = lib.rtw_last_error

    def call(p=None, w=W, h=H, i=img, o=out, none=False):
        p = _p() if p is None else p
        q = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        return fn(None if none else C.byref(p), w, h, q(i), q(o))

    assert call(none=True) == -1 and b"null" in err() and call(i=None) == -1 and call(o=None) == -1
    for bad in BAD_PARAMS:
        assert call(_p(**bad)) == -2, bad
    assert call(w=0) == -2 and call(h=-1) == -2
    assert call(o=img.view(np.uint8)) == -2 and b"alias" in err() and call(o=img.view(np.uint8)[img.nbytes - 1:]) == -2
    if not _has_gpu():
        assert call() not in (0, -1, -2, -5) and b"no HIP device" in err()


@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_render_presented_is_refused_without_a_device(lib, rtw, T, batch):
    """nulls (the filter's parameters may be null), the present stage's own checks, the filter's when it is given, and everything a feature
    render refuses"""
    from rtw_amd import _capi
    sfx = "f64" if T is np.float64 else "f32"
    fn = getattr(lib, ("rtw_render_presented_batch_" if batch else "rtw_render_presented_") + sfx)
    S, keep = _capi.make_scene(rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T), T)
    cams = _capi.make_cameras([rtw.t_default_cam(elem_type=T)] * 2, T)
    out = np.zeros(2 * 96 * 54 * 4, np.uint8)
    err = lib.rtw_last_error

    def call(P, p=None, d=None, scene=S, cm=cams, o=out, n=2, no_p=False):
        p = _p() if p is None else p
        views = (n, None) if batch else ()
        return fn(C.byref(scene) if scene is not None else None, cm, *views, C.byref(P) if P is not None else None, None if d is None else C.byref(d),
                  None if no_p else C.byref(p), o.ctypes.data_as(C.c_void_p) if o is not None else None)

    P = _capi.make_params(96, 54, 4)
    assert call(None) == -1 and call(P, scene=None) == -1 and call(P, cm=None) == -1 and call(P, o=None) == -1 and call(P, no_p=True) == -1
    assert b"null" in err()
    for bad in BAD_PARAMS:
        assert call(P, _p(**bad)) == -2, bad
    from rtw_amd.denoise import make_denoise
    assert call(P, d=make_denoise(levels=0)) == -2 and b"levels" in err() and call(P, d=make_denoise(sigma_color=0.0)) == -2
    if batch:
        assert call(P, n=0) == -2 and call(P, n=-3) == -2
    assert call(_capi.make_params(96, 54, 4, shard_index=0, shard_count=2)) == -2 and b"shard_count" in err()
    assert call(_capi.make_params(96, 54, 4, flags=_capi.FLAG_COMPACT_TILES)) == -2 and b"COMPACT_TILES" in err()
    assert call(_capi.make_params(96, 54, 4, devices=[0, 1])) == -2 and b"n_devices" in err()
    assert call(_capi.make_params(0, 54, 4)) == -2 and call(_capi.make_params(96, 0, 4)) == -2 and call(_capi.make_params(96, 54, 0)) == -2
    if not _has_gpu():
        assert call(P) not in (0, -1, -2, -5) and b"no HIP device" in err()
        assert call(P, d=make_denoise()) not in (0, -1, -2, -5) and b"no HIP device" in err()
    del keep


def test_python_validation(rtw):
    with pytest.raises(TypeError):
        rtw.present(np.zeros((3, 5, 3), np.int32))
    with pytest.raises(ValueError):
        rtw.present(np.zeros((3, 5, 4), np.float32))
    with pytest.raises(ValueError):
        rtw.present(np.zeros((0, 5, 3), np.float32))
    with pytest.raises(ValueError):
        rtw.make_present(channels=5)
    with pytest.raises(ValueError):
        rtw.make_present(nan_rgb=(0, 256, 0))
    with pytest.raises(ValueError):
        rtw.present_batch_into(0x1000, 0x2000, 5, 3, 0)
    with pytest.raises(TypeError):
        rtw.render_presented(rtw.scene_2_spheres(elem_type=np.float32), "not a camera", 96, 1)
    P = rtw.make_present(channels=4, dither=True, bgr=True, sqrt=True, exposure=0.5, nan_rgb=(1, 2, 3), device=0)
    assert (P.channels, P.flags, P.device, list(P.nan_rgb), P.reserved0, P.exposure, list(P.reserved)) == (4, 7, 0, [1, 2, 3], 0, 0.5, [0, 0])
    assert rtw.present_bytes(96, 54) == 96 * 54 * 3 and rtw.present_bytes(96, 54, 4, 3) == 96 * 54 * 12


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_present_fails_loudly_without_gpu(rtw):
    from rtw_amd._capi import RtwError
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.present(np.zeros((3, 5, 3), np.float32))
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.render_presented(rtw.scene_2_spheres(elem_type=np.float32), rtw.t_default_cam(elem_type=np.float32), 96, 4, denoise=True)


def test_c_presented_example_compiles_and_links(tmp_path):
    """examples/render_presented_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_presented_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "render_presented_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "4"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr and not (tmp_path / "render_presented_c.ppm").exists()
