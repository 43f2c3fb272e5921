"""The feature-guided denoiser, CPU only (include/rtw_hip.h rtw_denoise_*): the symbols are declared, listed and exported, the struct has
its 40 bytes, and every refusal is decided before any HIP call (the dummy device pointers below are never dereferenced)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

DENOISE_SYMBOLS = ["rtw_denoise_work_bytes", "rtw_denoise_device_f32", "rtw_denoise_device_f64", "rtw_denoise_f32", "rtw_denoise_f64",
                   "rtw_render_denoised_f32", "rtw_render_denoised_f64"]


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


def test_denoise_symbols_declared_exported_and_listed(lib, rtw):
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in DENOISE_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert sorted(n for n in declared if "denois" in n) == sorted(DENOISE_SYMBOLS)
    assert lib.rtw_abi_version() == 4                    # additive: the ABI version stays
    assert re.search(r"#define\s+RTW_DENOISE_DEMODULATE\s+1\b", header) and "RTW_DENOISE_DIRECT" not in header
    assert _capi.DENOISE_DEMODULATE == 1
    for name in ("denoise", "denoise_into", "denoise_work_bytes", "render_denoised"):
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name


def test_the_struct_has_40_bytes(tmp_path):
    from rtw_amd import _capi
    assert C.sizeof(_capi.Denoise) == 40
    assert _capi.Denoise.sigma_color.offset == 24 and _capi.Denoise.sigma_depth.offset == 32
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtw_hip.h"\n'
                   'int main(void) { printf("%d %d %d\\n", (int)sizeof(rtw_denoise_t), (int)offsetof(rtw_denoise_t, sigma_color), (int)offsetof(rtw_denoise_t, device)); return 0; }\n')
    exe = str(tmp_path / "size")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([exe], capture_output=True, text=True).stdout.split() == ["40", "24", "16"]


def test_work_bytes(lib):
    wb = lib.rtw_denoise_work_bytes
    prev = 0
    for w, h in ((1, 1), (2, 1), (2, 2), (5, 3), (37, 23), (70, 41), (1920, 1080), (3840, 2160)):
        for eb in (4, 8):
            n = wb(w, h, eb)
            assert n > 0 and n % 16 == 0, (w, h, eb, n)
        assert wb(w, h, 8) > wb(w, h, 4) >= prev                           # monotone in the size
        assert wb(w + 1, h, 4) >= wb(w, h, 4) and wb(w, h + 1, 4) >= wb(w, h, 4)
        prev = wb(w, h, 4)
    assert wb(1 << 17, 1 << 17, 8) == 2 ** 41                              # 64-bit: not truncated
    assert wb(5, 3, 2) == -2 and wb(5, 3, 0) == -2 and wb(5, 3, 16) == -2 and b"elem_bytes" in lib.rtw_last_error()
    assert wb(0, 3, 4) == -2 and wb(5, 0, 4) == -2 and wb(-1, 3, 4) == -2
    assert wb(2 ** 31 - 1, 2 ** 31 - 1, 4) == -5 and b"too large" in lib.rtw_last_error()


BAD_PARAMS = [dict(levels=0), dict(levels=9), dict(levels=-1), dict(normal_power_log2=-1), dict(normal_power_log2=8), dict(flags=2), dict(flags=4), dict(flags=-1),
              dict(gamma=2), dict(gamma=-1), dict(reserved=1), dict(device=-2), dict(sigma_color=0.0), dict(sigma_color=-1.0),
              dict(sigma_color=float("inf")), dict(sigma_color=float("nan")), dict(sigma_depth=0.0), dict(sigma_depth=-0.5),
              dict(sigma_depth=float("inf")), dict(sigma_depth=float("nan"))]


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_device_form_is_refused_without_a_device(lib, T):
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_denoise_device_" + sfx)
    W, H = 5, 3
    n_img, n_feat, n_work = W * H * 3 * eb, W * H * 8 * eb, lib.rtw_denoise_work_bytes(W, H, eb)
    img, feat, out, work = 0x100000, 0x200000, 0x300000, 0x400000       # never dereferenced
    err = lib.rtw_last_error

    def call(d=None, w=W, h=H, i=img, f=feat, o=out, k=work, none=False):
        d = _d() if d is None else d
        return fn(None if none else C.byref(d), w, h, C.c_void_p(i), C.c_void_p(f), C.c_void_p(o), C.c_void_p(k), None)

    assert call(none=True) == -1 and b"null" in err()
    assert call(i=0) == -1 and call(f=0) == -1 and call(o=0) == -1 and call(k=0) == -1
    for bad in BAD_PARAMS:
        assert call(_d(**bad)) == -2, bad
    assert call(w=0) == -2 and call(h=0) == -2 and call(w=-5) == -2
    assert call(w=2 ** 31 - 1, h=2 ** 31 - 1) == -5 and b"too large" in err()
    # alignment
    assert call(k=work + 8) == -2 and b"aligned" in err()
    assert call(f=feat + 8) == -2 and b"aligned" in err()
    assert call(i=img + 2) == -2 and call(o=out + 2) == -2
    # aliasing: the result against both inputs and the workspace, first and last byte
    assert call(o=img) == -2 and b"alias" in err()
    assert call(o=img + n_img - eb) == -2 and call(o=img - n_img + eb) == -2
    assert call(o=feat + n_feat - eb) == -2 and call(o=work + n_work - eb) == -2 and call(o=work) == -2
    assert call(k=img) == -2 and call(k=feat + 16) == -2
    # precedence: a null beats a bad parameter
    assert call(_d(levels=0), o=0) == -1
    if not _has_gpu():
        rc = call()                                     # everything in order: only the device is missing
        assert rc not in (0, -1, -2, -5)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_host_form_is_refused_without_a_device(lib, T):
    sfx = "f64" if T is np.float64 else "f32"
    fn = getattr(lib, "rtw_denoise_" + sfx)
    W, H = 5, 3
    buf = np.zeros(W * H * 16, T)
    img, feat, out = buf[:W * H * 3], buf[W * H * 3:W * H * 11], buf[W * H * 11:W * H * 14]
    err = lib.rtw_last_error

    def call(d=None, w=W, h=H, i=img, f=feat, o=out, none=False):
        d = _d() if d is None else d
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        return fn(None if none else C.byref(d), w, h, p(i), p(f), p(o))

    assert call(none=True) == -1 and b"null" in err()
    assert call(i=None) == -1 and call(f=None) == -1 and call(o=None) == -1
    for bad in BAD_PARAMS:
        assert call(_d(**bad)) == -2, bad
    assert call(w=0) == -2 and call(h=-1) == -2
    assert call(o=img) == -2 and b"alias" in err()
    assert call(o=buf[W * H * 3 - 1:]) == -2 and call(o=buf[W * H * 11 - 1:]) == -2
    if not _has_gpu():
        assert call() not in (0, -1, -2, -5) and b"no HIP device" in err()


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_render_denoised_is_refused_without_a_device(lib, rtw, T):
    """nulls, the denoiser's own checks, and everything a feature render refuses"""
    from rtw_amd import _capi
    sfx = "f64" if T is np.float64 else "f32"
    fn = getattr(lib, "rtw_render_denoised_" + sfx)
    S, keep = _capi.make_scene(rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T), T)
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    out = np.zeros(96 * 54 * 3, T)
    err = lib.rtw_last_error

    def call(P, d=None, scene=S, cm=cam, o=out, no_d=False):
        d = _d() if d is None else d
        return fn(C.byref(scene) if scene is not None else None, C.byref(cm) if cm is not None else None, C.byref(P) if P is not None else None,
                  None if no_d else C.byref(d), o.ctypes.data_as(C.c_void_p) if o is not None else None)

    P = _capi.make_params(96, 54, 4)
    assert call(None) == -1 and call(P, scene=None) == -1 and call(P, cm=None) == -1 and call(P, o=None) == -1 and call(P, no_d=True) == -1
    for bad in BAD_PARAMS:
        assert call(P, _d(**bad)) == -2, bad
    assert call(_capi.make_params(96, 54, 4, shard_index=0, shard_count=2)) == -2 and b"shard_count" in err()
    assert call(_capi.make_params(96, 54, 4, flags=_capi.FLAG_COMPACT_TILES)) == -2 and b"COMPACT_TILES" in err()
    assert call(_capi.make_params(96, 54, 4, flags=_capi.FLAG_RCCL_REDUCE)) == -2 and b"RCCL_REDUCE" in err()
    assert call(_capi.make_params(96, 54, 4, flags=_capi.FLAG_RAY_POOL)) == -2 and b"RAY_POOL" in err()
    assert call(_capi.make_params(96, 54, 4, devices=[0, 1])) == -2 and b"n_devices" in err()
    assert call(_capi.make_params(0, 54, 4)) == -2 and call(_capi.make_params(96, 0, 4)) == -2 and call(_capi.make_params(96, 54, 0)) == -2
    assert call(_capi.make_params(96, 54, 4, flags=64)) == -2 and b"unknown flags" in err()
    assert call(_capi.make_params(96, 54, 4, job_pixels=3)) == -2 and b"job_pixels" in err()
    if not _has_gpu():
        assert call(P) not in (0, -1, -2, -5) and b"no HIP device" in err()
    del keep


def test_python_validation(rtw):
    img, feat = np.zeros((3, 5, 3), np.float32), np.zeros((3, 5, 8), np.float32)
    with pytest.raises(TypeError):
        rtw.denoise(img, feat.astype(np.float64))
    with pytest.raises(TypeError):
        rtw.denoise(img.astype(np.int32), feat.astype(np.int32))
    with pytest.raises(ValueError):
        rtw.denoise(img, feat[:, :4])
    with pytest.raises(ValueError):
        rtw.denoise(img[..., :2], feat)
    with pytest.raises(ValueError):
        rtw.render_denoised(rtw.scene_2_spheres(elem_type=np.float32), rtw.t_default_cam(elem_type=np.float32), 96, 0)
    with pytest.raises(ValueError):
        rtw.denoise_into(0x1000, 0x2000, 0x3000, 0x4000, 5, 3, work_bytes=16)
    assert rtw.denoise_work_bytes(5, 3) == rtw.denoise_work_bytes(5, 3, np.float64) // 2 > 0


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_denoise_fails_loudly_without_gpu(rtw):
    from rtw_amd._capi import RtwError
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.denoise(np.zeros((3, 5, 3), np.float32), np.zeros((3, 5, 8), np.float32))
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.render_denoised(rtw.scene_2_spheres(elem_type=np.float32), rtw.t_default_cam(elem_type=np.float32), 96, 4)


def test_c_denoised_example_compiles_and_links(tmp_path):
    """examples/render_denoised_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_denoised_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "render_denoised_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "4"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr
