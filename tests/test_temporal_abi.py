"""Temporal reprojection, CPU only (include/rtw_hip.h rtw_temporal_*, rtw_render_sequence_*): the symbols are declared, listed and exported,
the struct has its 48 bytes, the state's size is what the header says, and every refusal of every entry point is decided before any HIP
call (the dummy device pointers below are never dereferenced)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

TEMPORAL_SYMBOLS = ["rtw_temporal_state_bytes", "rtw_temporal_device_f32", "rtw_temporal_device_f64", "rtw_temporal_f32", "rtw_temporal_f64",
                    "rtw_render_sequence_f32", "rtw_render_sequence_f64"]


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


def _t(**kw):
    from rtw_amd import _capi
    v = dict(normal_power_log2=1, flags=1, gamma=1, device=-1, reserved=(0, 0), sigma_depth=0.1, min_weight=0.25, history_max=16.0)
    v.update(kw)
    v["reserved"] = (C.c_int32 * 2)(*v["reserved"])
    return _capi.Temporal(**v)


def test_temporal_symbols_declared_exported_and_listed(lib, rtw):
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in TEMPORAL_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert sorted(n for n in declared if "temporal" in n or "sequence" in n) == sorted(TEMPORAL_SYMBOLS)
    assert lib.rtw_abi_version() == 4                    # additive: the ABI version stays
    assert re.search(r"#define\s+RTW_TEMPORAL_DEMODULATE\s+1\b", header) and _capi.TEMPORAL_DEMODULATE == 1
    for name in ("make_temporal", "temporal_state_bytes", "temporal_step", "temporal_step_into", "TemporalAccumulator", "render_sequence"):
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name
    # the denoiser's block no longer lists temporal reuse as out of scope, and DESIGN.md section 9 names what IS left out
    assert "Temporal reuse across the views of a batch, compact" not in header
    assert "Left out on purpose" in header


def test_the_struct_has_48_bytes(tmp_path):
    from rtw_amd import _capi
    S = _capi.Temporal
    assert C.sizeof(S) == 48
    assert S.device.offset == 12 and S.reserved.offset == 16 and S.sigma_depth.offset == 24 and S.min_weight.offset == 32 and S.history_max.offset == 40
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtw_hip.h"\n'
                   'int main(void) { printf("%d %d %d %d %d\\n", (int)sizeof(rtw_temporal_t), (int)offsetof(rtw_temporal_t, reserved), '
                   '(int)offsetof(rtw_temporal_t, sigma_depth), (int)offsetof(rtw_temporal_t, min_weight), (int)offsetof(rtw_temporal_t, history_max)); return 0; }\n')
    exe = str(tmp_path / "size")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([exe], capture_output=True, text=True).stdout.split() == ["48", "16", "24", "32", "40"]


def test_state_bytes(lib, rtw):
    sb = lib.rtw_temporal_state_bytes
    for w, h in ((1, 1), (5, 3), (37, 23), (70, 41), (1920, 1080), (1 << 15, 1 << 15)):
        for eb in (4, 8):
            n = sb(w, h, eb)
            assert n == (9 * w * h * eb + 15) // 16 * 16 and n % 16 == 0, (w, h, eb)
            assert (4 * w * h * eb) % 16 == 0 and (8 * w * h * eb) % 16 == 0         # the G and the L plane start on 16-byte boundaries
    assert sb(1, 1, 4) == 48 and sb(1, 1, 8) == 80 and sb(5, 3, 4) == 544
    last = 0
    for w in range(1, 40):                                # monotone in the size
        assert sb(w, 7, 4) >= last and sb(7, w, 4) == sb(w, 7, 4)
        last = sb(w, 7, 4)
    for args in ((5, 3, 2), (5, 3, 0), (5, 3, 16), (0, 3, 4), (5, 0, 4), (-1, 3, 4)):
        assert sb(*args) == -2, args
    assert sb(5, 3, 3) == -2 and b"elem_bytes" in lib.rtw_last_error()
    assert sb(2 ** 31 - 1, 2 ** 31 - 1, 8) == -5 and b"too large" in lib.rtw_last_error()
    assert rtw.temporal_state_bytes(5, 3) == 544 and rtw.temporal_state_bytes(5, 3, np.float64) == 1088
    from rtw_amd._capi import RtwError
    with pytest.raises(RtwError):
        rtw.temporal_state_bytes(0, 3)


BAD_PARAMS = [dict(normal_power_log2=-1), dict(normal_power_log2=8), dict(flags=2), dict(flags=4), dict(flags=-1), dict(gamma=2), dict(gamma=-1),
              dict(device=-2), dict(reserved=(1, 0)), dict(reserved=(0, -1)),
              dict(sigma_depth=0.0), dict(sigma_depth=-0.5), dict(sigma_depth=float("inf")), dict(sigma_depth=float("nan")),
              dict(min_weight=0.0), dict(min_weight=-0.25), dict(min_weight=1.5), dict(min_weight=float("inf")), dict(min_weight=float("nan")),
              dict(history_max=0.5), dict(history_max=0.0), dict(history_max=-3.0), dict(history_max=float("inf")), dict(history_max=float("nan"))]
GOOD_PARAMS = [dict(normal_power_log2=0), dict(normal_power_log2=7), dict(flags=0), dict(gamma=0), dict(min_weight=1.0), dict(min_weight=2.0 ** -30),
               dict(history_max=1.0), dict(history_max=1e6)]
#: (width, height) -> code
BAD_SIZES = [((0, 3), -2), ((5, 0), -2), ((-5, 3), -2), ((5, -3), -2), ((2 ** 31 - 1, 2 ** 31 - 1), -5)]


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_device_form_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_temporal_device_" + sfx)
    W, H = 10, 6
    n_img, n_feat, n_st = W * H * 3 * eb, W * H * 8 * eb, lib.rtw_temporal_state_bytes(W, H, eb)
    img, feat, sp, sn, out = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000       # never dereferenced
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    err = lib.rtw_last_error

    def call(t=None, size=(W, H), c=cam, cp=cam, i=img, f=feat, p=sp, n=sn, o=out, none=False):
        t = _t() if t is None else t
        ref = lambda x: None if x is None else C.byref(x)
        return fn(None if none else C.byref(t), ref(c), ref(cp), *size, C.c_void_p(i), C.c_void_p(f), C.c_void_p(p) if p else None, C.c_void_p(n), C.c_void_p(o), None)

    assert call(none=True) == -1 and b"null" in err()
    assert call(c=None) == -1 and call(i=0) == -1 and call(f=0) == -1 and call(n=0) == -1 and call(o=0) == -1
    for bad in BAD_PARAMS:
        assert call(_t(**bad)) == -2, bad
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    assert call(size=(2 ** 31 - 1, 2 ** 31 - 1)) == -5 and b"too large" in err()
    # exactly one of cam_prev / d_state_prev
    assert call(cp=None) == -2 and b"both" in err()
    assert call(p=0) == -2 and b"both" in err()
    # alignment
    assert call(f=feat + 8) == -2 and b"aligned" in err()
    assert call(p=sp + 8) == -2 and call(n=sn + 8) == -2 and b"aligned" in err()
    assert call(i=img + 2) == -2 and call(o=out + 2) == -2
    # aliasing: the result and the next state against each other and against the three inputs, first and last byte
    assert call(o=sn) == -2 and b"alias" in err()
    assert call(o=sn + n_st - eb) == -2 and call(o=sn - n_img + eb) == -2
    assert call(o=img) == -2 and call(o=img + n_img - eb) == -2 and call(o=img - n_img + eb) == -2
    assert call(o=feat + n_feat - eb) == -2 and call(o=sp + n_st - eb) == -2 and call(o=sp - n_img + eb) == -2
    assert call(n=img - n_st + 16) == -2 and call(n=feat + n_feat - 16) == -2 and call(n=sp) == -2 and call(n=sp + n_st - 16) == -2 and b"alias" in err()
    # precedence: a null beats a bad parameter
    assert call(_t(gamma=9), o=0) == -1
    if not _has_gpu():
        rc = call()                                     # everything in order: only the device is missing
        assert rc not in (0, -1, -2, -5)
        assert call(cp=None, p=0) == rc                 # the first frame is legal
        assert call(cp=None, p=0, o=sp) == rc           # ... and has no previous state to alias
        for good in GOOD_PARAMS:
            assert call(_t(**good)) == rc, good


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_host_form_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_temporal_" + sfx)
    W, H = 10, 6
    n, ns = W * H, lib.rtw_temporal_state_bytes(W, H, eb) // eb
    buf = np.zeros(n * 14 + 2 * ns + 8, T)
    img, feat, out = buf[:n * 3], buf[n * 3:n * 11], buf[n * 11:n * 14]
    sp, sn = buf[n * 14:n * 14 + ns], buf[n * 14 + ns:n * 14 + 2 * ns]
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    err = lib.rtw_last_error

    def call(t=None, size=(W, H), c=cam, cp=cam, i=img, f=feat, p=sp, nx=sn, o=out, none=False):
        t = _t() if t is None else t
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        ref = lambda x: None if x is None else C.byref(x)
        return fn(None if none else C.byref(t), ref(c), ref(cp), *size, ptr(i), ptr(f), ptr(p), ptr(nx), ptr(o))

    assert call(none=True) == -1 and b"null" in err()
    assert call(c=None) == -1 and call(i=None) == -1 and call(f=None) == -1 and call(nx=None) == -1 and call(o=None) == -1
    for bad in BAD_PARAMS:
        assert call(_t(**bad)) == -2, bad
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    assert call(cp=None) == -2 and b"both" in err()
    assert call(p=None) == -2 and b"both" in err()
    assert call(o=img) == -2 and b"alias" in err()
    assert call(o=buf[n * 3 - 1:]) == -2 and call(o=buf[n * 11 - 1:]) == -2 and call(o=buf[n * 14 - 1:]) == -2 and call(o=buf[n * 14 + ns:]) == -2
    assert call(nx=sp) == -2 and call(nx=buf[n * 3 - 1:]) == -2 and call(nx=buf[n * 14 + 1:]) == -2 and b"alias" in err()
    assert call(_t(gamma=9), o=None) == -1
    if not _has_gpu():
        assert call() not in (0, -1, -2, -5) and b"no HIP device" in err()
        assert call(cp=None, p=None) not in (0, -1, -2, -5)


@pytest.mark.parametrize("with_d", [False, True])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_render_sequence_is_refused_without_a_device(lib, rtw, T, with_d):
    """nulls, the step's own checks, the filter's (when given), and everything a batched feature render refuses"""
    from rtw_amd import _capi
    sfx = "f64" if T is np.float64 else "f32"
    fn = getattr(lib, "rtw_render_sequence_" + sfx)
    S, keep = _capi.make_scene(rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T), T)
    N = 3
    cams = _capi.make_cameras([rtw.t_default_cam(elem_type=T)] * N, T)
    out = np.zeros(N * 96 * 54 * 3, T)
    D = _capi.Denoise(3, 1, 1, 1, -1, 0, 0.5, 0.1)
    err = lib.rtw_last_error

    def call(P, t=None, d=D, scene=S, cm=cams, o=out, no_t=False, n=N):
        t = _t() if t is None else t
        return fn(C.byref(scene) if scene is not None else None, cm, n, None, C.byref(P) if P is not None else None, None if no_t else C.byref(t),
                  C.byref(d) if (with_d and d is not None) else None, o.ctypes.data_as(C.c_void_p) if o is not None else None)

    P = _capi.make_params(96, 54, 4)
    assert call(None) == -1 and call(P, scene=None) == -1 and call(P, cm=None) == -1 and call(P, o=None) == -1 and call(P, no_t=True) == -1
    for bad in BAD_PARAMS:
        assert call(P, _t(**bad)) == -2, bad
    if with_d:
        for bad in (dict(levels=0), dict(levels=9), dict(normal_power_log2=8), dict(flags=2), dict(gamma=2), dict(reserved=1), dict(device=-2),
                    dict(sigma_color=0.0), dict(sigma_depth=float("nan"))):
            v = dict(levels=3, normal_power_log2=1, flags=1, gamma=1, device=-1, reserved=0, sigma_color=0.5, sigma_depth=0.1)
            v.update(bad)
            assert call(P, d=_capi.Denoise(**v)) == -2, bad
    # what a batched feature render refuses
    assert call(_capi.make_params(96, 54, 4, shard_index=0, shard_count=2)) == -2 and b"shard_count" in err()
    assert call(_capi.make_params(96, 54, 4, flags=_capi.FLAG_COMPACT_TILES)) == -2 and b"COMPACT_TILES" in err()
    assert call(_capi.make_params(96, 54, 4, flags=_capi.FLAG_RCCL_REDUCE)) == -2 and b"RCCL_REDUCE" in err()
    assert call(_capi.make_params(96, 54, 4, flags=_capi.FLAG_RAY_POOL)) == -2 and b"RAY_POOL" in err()
    assert call(_capi.make_params(96, 54, 4, devices=[0, 1])) == -2 and b"n_devices" in err()
    assert call(_capi.make_params(0, 54, 4)) == -2 and call(_capi.make_params(96, 0, 4)) == -2 and call(_capi.make_params(96, 54, 0)) == -2
    assert call(_capi.make_params(96, 54, 4, flags=64)) == -2 and b"unknown flags" in err()
    assert call(_capi.make_params(96, 54, 4, job_pixels=3)) == -2 and b"job_pixels" in err()
    assert call(_capi.make_params(2 ** 31 - 1, 2 ** 31 - 1, 4)) == -5
    assert call(P, n=0) == -2 and call(P, n=-2) == -2 and b"n_views" in err()
    assert call(None, _t(gamma=9)) == -1                        # a null beats a bad parameter
    if not _has_gpu():
        assert call(P) not in (0, -1, -2, -5) and b"no HIP device" in err()
        assert call(P, n=1) not in (0, -1, -2, -5)
    del keep


def test_python_validation(rtw):
    T = np.float32
    img, feat = np.zeros((3, 5, 3), T), np.zeros((3, 5, 8), T)
    cam, cam64 = rtw.t_default_cam(elem_type=T), rtw.t_default_cam(elem_type=np.float64)
    n_state = rtw.temporal_state_bytes(5, 3) // 4
    with pytest.raises(TypeError):
        rtw.temporal_step(img, feat.astype(np.float64), cam)
    with pytest.raises(TypeError):
        rtw.temporal_step(img.astype(np.int32), feat.astype(np.int32), cam)
    with pytest.raises(TypeError):
        rtw.temporal_step(img, feat, cam64)
    with pytest.raises(TypeError):
        rtw.temporal_step(img, feat, "cam")
    with pytest.raises(ValueError):
        rtw.temporal_step(img, feat[:, :4], cam)
    with pytest.raises(ValueError):
        rtw.temporal_step(img[:0], feat[:0], cam)
    with pytest.raises(ValueError, match="both"):
        rtw.temporal_step(img, feat, cam, state=np.zeros(n_state, T))
    with pytest.raises(ValueError, match="both"):
        rtw.temporal_step(img, feat, cam, cam_prev=cam)
    with pytest.raises(ValueError, match="state must be"):
        rtw.temporal_step(img, feat, cam, state=np.zeros(n_state + 1, T), cam_prev=cam)
    with pytest.raises(ValueError, match="state must be"):
        rtw.temporal_step(img, feat, cam, state=np.zeros(n_state, np.float64), cam_prev=cam)
    with pytest.raises(TypeError):
        rtw.temporal_step(img, feat, cam, state=np.zeros(n_state, T), cam_prev=cam64)
    with pytest.raises(ValueError, match="both"):
        rtw.temporal_step_into(0x1000, 0x2000, 0x3000, 0x4000, cam, 5, 3, cam_prev=cam)
    with pytest.raises(ValueError, match="both"):
        rtw.temporal_step_into(0x1000, 0x2000, 0x3000, 0x4000, cam, 5, 3, d_state_prev_ptr=0x5000)
    with pytest.raises(TypeError):
        rtw.temporal_step_into(0x1000, 0x2000, 0x3000, 0x4000, cam64, 5, 3)
    scene = rtw.scene_2_spheres(elem_type=T)
    with pytest.raises(ValueError):
        rtw.render_sequence(scene, [], 96, 4)
    with pytest.raises(TypeError):
        rtw.render_sequence(scene, [cam, cam64], 96, 4)
    with pytest.raises(ValueError):
        rtw.render_sequence(scene, [cam, cam], 96, 0)
    with pytest.raises(ValueError):
        rtw.render_sequence(scene, [cam, cam], 96, 4, seeds=[1])
    with pytest.raises(ValueError, match="keywords"):
        rtw.render_sequence(scene, [cam, cam], 96, 4, denoise=dict(gamma=False))
    tp = rtw.make_temporal()
    assert (tp.normal_power_log2, tp.flags, tp.gamma, tp.device, tuple(tp.reserved)) == (1, 1, 1, -1, (0, 0))
    assert (tp.sigma_depth, tp.min_weight, tp.history_max) == (0.1, 0.25, 16.0)
    tp = rtw.make_temporal(3, 0.5, 0.5, 4, False, False, 2)
    assert (tp.normal_power_log2, tp.flags, tp.gamma, tp.device, tp.sigma_depth, tp.min_weight, tp.history_max) == (3, 0, 0, 2, 0.5, 0.5, 4.0)
    import rtw_amd.temporal
    assert "untuned" in rtw.make_temporal.__doc__ and "untuned" in rtw.render_sequence.__doc__ and "UNTUNED" in rtw_amd.temporal.__doc__


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_temporal_fails_loudly_without_gpu(rtw):
    from rtw_amd._capi import RtwError
    T = np.float32
    cam = rtw.t_default_cam(elem_type=T)
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.temporal_step(np.zeros((3, 5, 3), T), np.zeros((3, 5, 8), T), cam)
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.render_sequence(rtw.scene_2_spheres(elem_type=T), [cam, cam], 96, 4)


def test_c_sequence_example_compiles_and_links(tmp_path):
    """examples/render_sequence_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_sequence_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "render_sequence_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "2", "4"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr
