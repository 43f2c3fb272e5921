"""The feature-guided upsampler, CPU only (include/rtw_hip.h rtw_upsample_*): the symbols are declared, listed and exported, the struct has
its 48 bytes, and every refusal of every entry point is decided before any HIP call (the dummy device pointers below are never
dereferenced)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

UPSAMPLE_SYMBOLS = ["rtw_upsample_work_bytes", "rtw_upsample_device_f32", "rtw_upsample_device_f64", "rtw_upsample_f32", "rtw_upsample_f64",
                    "rtw_upsample_batch_device_f32", "rtw_upsample_batch_device_f64", "rtw_upsample_batch_f32", "rtw_upsample_batch_f64",
                    "rtw_render_upsampled_f32", "rtw_render_upsampled_f64", "rtw_render_upsampled_batch_f32", "rtw_render_upsampled_batch_f64"]


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


def _u(**kw):
    from rtw_amd import _capi
    v = dict(levels=2, normal_power_log2=1, flags=1, gamma=1, device=-1, hi_chunks=0, sigma_color=0.5, sigma_depth=0.1, sigma_albedo=0.2)
    v.update(kw)
    return _capi.Upsample(**v)


def test_upsample_symbols_declared_exported_and_listed(lib, rtw):
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in UPSAMPLE_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert sorted(n for n in declared if "upsampl" in n) == sorted(UPSAMPLE_SYMBOLS)
    assert lib.rtw_abi_version() == 4                    # additive: the ABI version stays
    assert re.search(r"#define\s+RTW_UPSAMPLE_DEMODULATE\s+1\b", header) and _capi.UPSAMPLE_DEMODULATE == 1
    for name in ("make_upsample", "upsample_work_bytes", "upsample", "upsample_into", "upsample_batch", "upsample_batch_into", "render_upsampled",
                 "render_upsampled_batch"):
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name


def test_the_struct_has_48_bytes(tmp_path):
    from rtw_amd import _capi
    U = _capi.Upsample
    assert C.sizeof(U) == 48
    assert U.hi_chunks.offset == 20 and U.sigma_color.offset == 24 and U.sigma_depth.offset == 32 and U.sigma_albedo.offset == 40
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtw_hip.h"\n'
                   'int main(void) { printf("%d %d %d %d\\n", (int)sizeof(rtw_upsample_t), (int)offsetof(rtw_upsample_t, sigma_color), '
                   '(int)offsetof(rtw_upsample_t, hi_chunks), (int)offsetof(rtw_upsample_t, sigma_albedo)); return 0; }\n')
    exe = str(tmp_path / "size")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([exe], capture_output=True, text=True).stdout.split() == ["48", "24", "20", "40"]


def test_work_bytes_are_the_denoisers_of_the_small_frame(lib):
    up, dn = lib.rtw_upsample_work_bytes, lib.rtw_denoise_work_bytes
    for w, h in ((1, 1), (5, 3), (18, 10), (35, 20), (960, 540), (1 << 17, 1 << 17)):
        for eb in (4, 8):
            assert up(w, h, eb) == dn(w, h, eb) > 0, (w, h, eb)
    for args in ((5, 3, 2), (5, 3, 0), (5, 3, 16), (0, 3, 4), (5, 0, 4), (-1, 3, 4), (2 ** 31 - 1, 2 ** 31 - 1, 4)):
        assert up(*args) == dn(*args) < 0, args
    assert up(5, 3, 3) == -2 and b"elem_bytes" in lib.rtw_last_error()
    assert up(2 ** 31 - 1, 2 ** 31 - 1, 8) == -5 and b"too large" in lib.rtw_last_error()


BAD_PARAMS = [dict(levels=-1), dict(levels=9), dict(normal_power_log2=-1), dict(normal_power_log2=8), dict(flags=2), dict(flags=4), dict(flags=-1),
              dict(gamma=2), dict(gamma=-1), dict(device=-2), dict(hi_chunks=-1),
              dict(sigma_color=0.0), dict(sigma_color=-1.0), dict(sigma_color=float("inf")), dict(sigma_color=float("nan")),
              dict(sigma_color=0.0, levels=0), dict(sigma_color=float("nan"), levels=0),
              dict(sigma_depth=0.0), dict(sigma_depth=-0.5), dict(sigma_depth=float("inf")), dict(sigma_depth=float("nan")),
              dict(sigma_albedo=0.0), dict(sigma_albedo=-0.5), dict(sigma_albedo=float("inf")), dict(sigma_albedo=float("nan"))]
#: (lo_width, lo_height, width, height) -> code
BAD_SIZES = [((0, 3, 10, 6), -2), ((5, 0, 10, 6), -2), ((5, 3, 0, 6), -2), ((5, 3, 10, 0), -2), ((-5, 3, 10, 6), -2), ((5, 3, 10, -6), -2),
             ((11, 3, 10, 6), -2), ((5, 7, 10, 6), -2), ((11, 7, 10, 6), -2),
             ((5, 3, 2 ** 31 - 1, 2 ** 31 - 1), -5), ((2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), -5)]


@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_device_forms_are_refused_without_a_device(lib, T, batch):
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, ("rtw_upsample_batch_device_" if batch else "rtw_upsample_device_") + sfx)
    w, h, W, H, N = 5, 3, 10, 6, (3 if batch else 1)
    n_img, n_flo, n_fhi, n_out = N * w * h * 3 * eb, N * w * h * 8 * eb, N * W * H * 8 * eb, N * W * H * 3 * eb
    n_work = N * lib.rtw_upsample_work_bytes(w, h, eb)
    img, flo, fhi, out, work = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000       # never dereferenced
    err = lib.rtw_last_error

    def call(u=None, size=(w, h, W, H), i=img, fl=flo, fh=fhi, o=out, k=work, none=False, n=N):
        u = _u() if u is None else u
        views = (n,) if batch else ()
        return fn(None if none else C.byref(u), *size, *views, C.c_void_p(i), C.c_void_p(fl), C.c_void_p(fh), C.c_void_p(o), C.c_void_p(k), None)

    assert call(none=True) == -1 and b"null" in err()
    assert call(i=0) == -1 and call(fl=0) == -1 and call(fh=0) == -1 and call(o=0) == -1 and call(k=0) == -1
    for bad in BAD_PARAMS:
        assert call(_u(**bad)) == -2, bad
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    assert call(size=(11, 3, 10, 6)) == -2 and b"exceed" in err()
    assert call(size=(5, 3, 2 ** 31 - 1, 2 ** 31 - 1)) == -5 and b"too large" in err()
    if batch:
        assert call(n=0) == -2 and call(n=-3) == -2 and b"n_views" in err()
        assert call(size=(5, 3, 1 << 17, 1 << 17), n=1 << 5) == -5 and b"too large" in err()
    # alignment
    assert call(k=work + 8) == -2 and b"aligned" in err()
    assert call(fl=flo + 8) == -2 and b"aligned" in err()
    assert call(fh=fhi + 8) == -2 and b"aligned" in err()
    assert call(i=img + 2) == -2 and call(o=out + 2) == -2
    # aliasing: the result against the three inputs and the workspace, first and last byte; the workspace against the inputs
    assert call(o=img) == -2 and b"alias" in err()
    assert call(o=img + n_img - eb) == -2 and call(o=img - n_out + eb) == -2
    assert call(o=flo + n_flo - eb) == -2 and call(o=fhi + n_fhi - eb) == -2 and call(o=fhi - n_out + eb) == -2
    assert call(o=work + n_work - eb) == -2 and call(o=work) == -2
    assert call(k=img) == -2 and call(k=flo + 16) == -2 and call(k=fhi + n_fhi - 16) == -2 and b"alias" in err()
    # precedence: a null beats a bad parameter
    assert call(_u(levels=9), o=0) == -1
    if not _has_gpu():
        rc = call()                                     # everything in order: only the device is missing
        assert rc not in (0, -1, -2, -5)
        assert call(_u(levels=0)) == rc and call(size=(10, 6, 10, 6)) == rc          # levels = 0 and equal sizes are legal


@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_host_forms_are_refused_without_a_device(lib, T, batch):
    sfx = "f64" if T is np.float64 else "f32"
    fn = getattr(lib, ("rtw_upsample_batch_" if batch else "rtw_upsample_") + sfx)
    w, h, W, H, N = 5, 3, 10, 6, (3 if batch else 1)
    lo, hi = N * w * h, N * W * H
    buf = np.zeros(lo * 11 + hi * 11 + 8, T)
    img, flo, fhi, out = buf[:lo * 3], buf[lo * 3:lo * 11], buf[lo * 11:lo * 11 + hi * 8], buf[lo * 11 + hi * 8:lo * 11 + hi * 11]
    err = lib.rtw_last_error

    def call(u=None, size=(w, h, W, H), i=img, fl=flo, fh=fhi, o=out, none=False, n=N):
        u = _u() if u is None else u
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        views = (n,) if batch else ()
        return fn(None if none else C.byref(u), *size, *views, p(i), p(fl), p(fh), p(o))

    assert call(none=True) == -1 and b"null" in err()
    assert call(i=None) == -1 and call(fl=None) == -1 and call(fh=None) == -1 and call(o=None) == -1
    for bad in BAD_PARAMS:
        assert call(_u(**bad)) == -2, bad
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    if batch:
        assert call(n=0) == -2 and call(n=-1) == -2
    assert call(o=img) == -2 and b"alias" in err()
    assert call(o=buf[lo * 3 - 1:]) == -2 and call(o=buf[lo * 11 - 1:]) == -2 and call(o=buf[lo * 11 + hi * 8 - 1:]) == -2
    assert call(_u(levels=9), o=None) == -1
    if not _has_gpu():
        assert call() not in (0, -1, -2, -5) and b"no HIP device" in err()


@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_render_upsampled_is_refused_without_a_device(lib, rtw, T, batch):
    """nulls, the upsampler's own checks, hi_chunks against the full render's chunks, and everything a feature render of p and of q refuses"""
    from rtw_amd import _capi
    sfx = "f64" if T is np.float64 else "f32"
    fn = getattr(lib, ("rtw_render_upsampled_batch_" if batch else "rtw_render_upsampled_") + sfx)
    S, keep = _capi.make_scene(rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T), T)
    N = 3 if batch else 1
    cams = _capi.make_cameras([rtw.t_default_cam(elem_type=T)] * N, T)
    out = np.zeros(N * 96 * 54 * 3, T)
    err = lib.rtw_last_error

    def call(P, u=None, lo=(48, 27), scene=S, cm=cams, o=out, no_u=False, n=N):
        u = _u() if u is None else u
        views = (n, None) if batch else ()
        return fn(C.byref(scene) if scene is not None else None, cm, *views, C.byref(P) if P is not None else None, *lo,
                  None if no_u else C.byref(u), o.ctypes.data_as(C.c_void_p) if o is not None else None)

    P = _capi.make_params(96, 54, 4)
    assert call(None) == -1 and call(P, scene=None) == -1 and call(P, cm=None) == -1 and call(P, o=None) == -1 and call(P, no_u=True) == -1
    for bad in BAD_PARAMS:
        assert call(P, _u(**bad)) == -2, bad
    # the small frame: sizes < 1 (q's own validation), larger than the full one in either direction
    assert call(P, lo=(0, 27)) == -2 and call(P, lo=(48, 0)) == -2 and call(P, lo=(-1, 27)) == -2
    assert call(P, lo=(97, 27)) == -2 and b"exceed" in err()
    assert call(P, lo=(48, 55)) == -2 and b"exceed" in err()
    # hi_chunks: 4 spp are 4 chunks
    assert call(P, _u(hi_chunks=5)) == -2 and b"chunk" in err()
    assert call(_capi.make_params(96, 54, 4, n_chunks=2), _u(hi_chunks=3)) == -2 and b"chunk" in err()
    # what a feature render refuses
    assert call(_capi.make_params(96, 54, 4, shard_index=0, shard_count=2)) == -2 and b"shard_count" in err()
    assert call(_capi.make_params(96, 54, 4, flags=_capi.FLAG_COMPACT_TILES)) == -2 and b"COMPACT_TILES" in err()
    assert call(_capi.make_params(96, 54, 4, flags=_capi.FLAG_RCCL_REDUCE)) == -2 and b"RCCL_REDUCE" in err()
    assert call(_capi.make_params(96, 54, 4, flags=_capi.FLAG_RAY_POOL)) == -2 and b"RAY_POOL" in err()
    assert call(_capi.make_params(96, 54, 4, devices=[0, 1])) == -2 and b"n_devices" in err()
    assert call(_capi.make_params(0, 54, 4)) == -2 and call(_capi.make_params(96, 0, 4)) == -2 and call(_capi.make_params(96, 54, 0)) == -2
    assert call(_capi.make_params(96, 54, 4, flags=64)) == -2 and b"unknown flags" in err()
    assert call(_capi.make_params(96, 54, 4, job_pixels=3)) == -2 and b"job_pixels" in err()
    assert call(_capi.make_params(2 ** 31 - 1, 2 ** 31 - 1, 4)) == -5
    if batch:
        assert call(P, n=0) == -2 and call(P, n=-2) == -2 and b"n_views" in err()
    assert call(None, _u(levels=9)) == -1                       # a null beats a bad parameter
    if not _has_gpu():
        assert call(P) not in (0, -1, -2, -5) and b"no HIP device" in err()
        assert call(P, _u(hi_chunks=4, levels=0)) not in (0, -1, -2, -5)
    del keep


def test_python_validation(rtw):
    lo, flo, fhi = np.zeros((3, 5, 3), np.float32), np.zeros((3, 5, 8), np.float32), np.zeros((6, 10, 8), np.float32)
    with pytest.raises(TypeError):
        rtw.upsample(lo, flo, fhi.astype(np.float64))
    with pytest.raises(TypeError):
        rtw.upsample(lo.astype(np.int32), flo.astype(np.int32), fhi.astype(np.int32))
    with pytest.raises(ValueError):
        rtw.upsample(lo, flo[:, :4], fhi)
    with pytest.raises(ValueError):
        rtw.upsample(lo, flo, fhi[..., :7])
    with pytest.raises(ValueError, match="exceeds"):
        rtw.upsample(lo, flo, fhi[:2])
    with pytest.raises(ValueError):
        rtw.upsample_batch(lo[None], flo[None], np.zeros((2, 6, 10, 8), np.float32))
    scene, cam = rtw.scene_2_spheres(elem_type=np.float32), rtw.t_default_cam(elem_type=np.float32)
    with pytest.raises(ValueError):
        rtw.render_upsampled(scene, cam, 96, 0)
    with pytest.raises(ValueError):
        rtw.render_upsampled(scene, cam, 96, 4, lo_width=97)
    with pytest.raises(ValueError):
        rtw.render_upsampled(scene, cam, 96, 4, lo_width=1)             # a small frame 1 wide is 0 high
    with pytest.raises(ValueError):
        rtw.upsample_into(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 5, 3, 10, 6, work_bytes=16)
    with pytest.raises(ValueError):
        rtw.upsample_batch_into(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 5, 3, 10, 6, 0)
    assert rtw.upsample_work_bytes(5, 3) == rtw.denoise_work_bytes(5, 3) == rtw.upsample_work_bytes(5, 3, np.float64) // 2 > 0
    U = rtw.make_upsample()
    assert (U.levels, U.normal_power_log2, U.flags, U.gamma, U.device, U.hi_chunks) == (2, 1, 1, 1, -1, 0)
    assert (U.sigma_color, U.sigma_depth, U.sigma_albedo) == (0.5, 0.1, 0.2)
    assert "untuned" in rtw.make_upsample.__doc__ and "untuned" in rtw.render_upsampled.__doc__


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_upsample_fails_loudly_without_gpu(rtw):
    from rtw_amd._capi import RtwError
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.upsample(np.zeros((3, 5, 3), np.float32), np.zeros((3, 5, 8), np.float32), np.zeros((6, 10, 8), np.float32))
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.render_upsampled(rtw.scene_2_spheres(elem_type=np.float32), rtw.t_default_cam(elem_type=np.float32), 96, 4)


def test_c_upsampled_example_compiles_and_links(tmp_path):
    """examples/render_upsampled_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_upsampled_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "render_upsampled_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "4"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr
