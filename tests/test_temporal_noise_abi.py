"""Temporal moments, CPU only (include/rtw_hip.h rtw_history_moment_bytes, rtw_history_moments_*, rtw_history_noise_device_*,
rtw_render_path_guided_*): the symbols are declared, listed and exported, the struct has its 40 bytes, the moment plane's size is what the
header says, and every refusal of every new entry point is decided before any HIP call (the dummy device pointers below are never
dereferenced)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NOISE_SYMBOLS = ["rtw_history_moment_bytes", "rtw_history_moments_device_f32", "rtw_history_moments_device_f64", "rtw_history_noise_device_f32",
                 "rtw_history_noise_device_f64", "rtw_history_moments_f32", "rtw_history_moments_f64", "rtw_render_path_guided_f32",
                 "rtw_render_path_guided_f64"]


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


def _n(**kw):
    from rtw_amd import _capi
    v = dict(radius=2, normal_power_log2=1, device=-1, reserved=(0, 0, 0), sigma_depth=0.1, min_len=4.0)
    v.update(kw)
    v["reserved"] = (C.c_int32 * 3)(*v["reserved"])
    return _capi.TemporalNoise(**v)


def test_symbols_declared_exported_and_listed(lib, rtw):
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NOISE_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert sorted(n for n in declared if "history" in n or "path_guided" in n) == sorted(NOISE_SYMBOLS)
    # tests/test_temporal_abi.py pins the declared names that contain "temporal" or "sequence" to the plain step's seven: the new ones carry neither
    assert not any("temporal" in n or "sequence" in n for n in NOISE_SYMBOLS)
    assert lib.rtw_abi_version() == 4                    # additive: the ABI version stays
    assert "rtw_temporal_noise_t" in header and not re.search(r"#define\s+RTW_FLAG_[A-Z_]*(MOMENT|NOISE)", header)
    for name in ("make_temporal_noise", "temporal_moment_bytes", "temporal_step_moments", "temporal_step_moments_into", "temporal_noise_into"):
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name
    assert "UNTUNED" in header[header.index("Temporal moments"):]


def test_the_struct_has_40_bytes(tmp_path):
    from rtw_amd import _capi
    S = _capi.TemporalNoise
    assert C.sizeof(S) == 40
    assert S.radius.offset == 0 and S.normal_power_log2.offset == 4 and S.device.offset == 8 and S.reserved.offset == 12 and S.sigma_depth.offset == 24 and S.min_len.offset == 32
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtw_hip.h"\n'
                   'int main(void) { printf("%d %d %d %d %d %d\\n", (int)sizeof(rtw_temporal_noise_t), (int)offsetof(rtw_temporal_noise_t, device), '
                   '(int)offsetof(rtw_temporal_noise_t, reserved), (int)offsetof(rtw_temporal_noise_t, sigma_depth), (int)offsetof(rtw_temporal_noise_t, min_len), '
                   '(int)sizeof(rtw_temporal_t)); return 0; }\n')
    exe = str(tmp_path / "size")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([exe], capture_output=True, text=True).stdout.split() == ["40", "8", "12", "24", "32", "48"]


def test_moment_bytes(lib, rtw):
    mb, sb = lib.rtw_history_moment_bytes, lib.rtw_temporal_state_bytes
    for w, h in ((1, 1), (3, 2), (5, 3), (70, 40), (1920, 1080), (1 << 15, 1 << 15)):
        for eb in (4, 8):
            n = mb(w, h, eb)
            assert n == (w * h * eb + 15) // 16 * 16 and n % 16 == 0, (w, h, eb)
            assert sb(w, h, eb) == (9 * w * h * eb + 15) // 16 * 16                   # the public state keeps its size
    assert mb(1, 1, 4) == 16 and mb(1, 1, 8) == 16 and mb(5, 3, 4) == 64 and mb(5, 3, 8) == 128
    last = 0
    for w in range(1, 40):                                # monotone in the size
        assert mb(w, 7, 4) >= last and mb(7, w, 4) == mb(w, 7, 4)
        last = mb(w, 7, 4)
    for args in ((5, 3, 2), (5, 3, 0), (5, 3, 16), (0, 3, 4), (5, 0, 4), (-1, 3, 4), (2 ** 31 - 1, 2 ** 31 - 1, 8)):
        assert mb(*args) == sb(*args) and mb(*args) < 0, args     # the same error codes
    assert mb(5, 3, 3) == -2 and b"elem_bytes" in lib.rtw_last_error()
    assert mb(2 ** 31 - 1, 2 ** 31 - 1, 8) == -5 and b"too large" in lib.rtw_last_error()
    assert rtw.temporal_moment_bytes(5, 3) == 64 and rtw.temporal_moment_bytes(5, 3, np.float64) == 128
    from rtw_amd._capi import RtwError
    with pytest.raises(RtwError):
        rtw.temporal_moment_bytes(0, 3)


BAD_T = [dict(normal_power_log2=-1), dict(normal_power_log2=8), dict(flags=2), dict(flags=-1), dict(gamma=2), dict(device=-2), dict(reserved=(1, 0)), dict(reserved=(0, -1)),
         dict(sigma_depth=0.0), dict(sigma_depth=float("nan")), dict(min_weight=0.0), dict(min_weight=1.5), dict(history_max=0.5), dict(history_max=float("inf"))]
BAD_N = [dict(radius=0), dict(radius=4), dict(radius=-1), dict(normal_power_log2=-1), dict(normal_power_log2=8), dict(device=-2),
         dict(reserved=(1, 0, 0)), dict(reserved=(0, -1, 0)), dict(reserved=(0, 0, 7)),
         dict(sigma_depth=0.0), dict(sigma_depth=-0.5), dict(sigma_depth=float("inf")), dict(sigma_depth=float("nan")),
         dict(min_len=0.5), dict(min_len=0.0), dict(min_len=-3.0), dict(min_len=float("inf")), dict(min_len=float("nan"))]
GOOD_N = [dict(radius=1), dict(radius=3), dict(normal_power_log2=0), dict(normal_power_log2=7), dict(min_len=1.0), dict(min_len=1e6), dict(sigma_depth=1e-6)]
BAD_SIZES = [((0, 3), -2), ((5, 0), -2), ((-5, 3), -2), ((5, -3), -2), ((2 ** 31 - 1, 2 ** 31 - 1), -5)]


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_moment_step_device_form_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_history_moments_device_" + sfx)
    W, H = 10, 6
    n_img, n_feat, n_st, n_mo = W * H * 3 * eb, W * H * 8 * eb, lib.rtw_temporal_state_bytes(W, H, eb), lib.rtw_history_moment_bytes(W, H, eb)
    img, feat, sp, sn, out, mp, mn = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000       # never dereferenced
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    err = lib.rtw_last_error
    vp = lambda x: C.c_void_p(x) if x else None

    def call(t=None, size=(W, H), c=cam, cp=cam, i=img, f=feat, p=sp, q=mp, n=sn, m=mn, o=out, none=False):
        t = _t() if t is None else t
        ref = lambda x: None if x is None else C.byref(x)
        return fn(None if none else C.byref(t), ref(c), ref(cp), *size, vp(i), vp(f), vp(p), vp(q), vp(n), vp(m), vp(o), None)

    assert call(none=True) == -1 and b"null" in err()
    assert call(c=None) == -1 and call(i=0) == -1 and call(f=0) == -1 and call(n=0) == -1 and call(o=0) == -1 and call(m=0) == -1
    for bad in BAD_T:
        assert call(_t(**bad)) == -2, bad
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    # cam_prev, d_state_prev and d_moment_prev are null together
    assert call(cp=None) == -2 and b"both" in err()
    assert call(p=0) == -2 and b"both" in err()
    assert call(q=0) == -2 and b"d_moment_prev" in err()
    assert call(cp=None, p=0) == -2 and b"d_moment_prev" in err()
    # alignment
    assert call(f=feat + 8) == -2 and call(p=sp + 8) == -2 and call(n=sn + 8) == -2 and b"aligned" in err()
    assert call(q=mp + 8) == -2 and b"moment" in err() and call(m=mn + 4) == -2 and b"aligned" in err()
    assert call(i=img + 2) == -2 and call(o=out + 2) == -2
    # aliasing: the rules of the plain step ...
    assert call(o=sn) == -2 and b"alias" in err()
    assert call(o=img + n_img - eb) == -2 and call(o=sp + n_st - eb) == -2 and call(n=sp) == -2 and call(n=feat + n_feat - 16) == -2
    # ... extended to the moment planes: the next one against the other outputs and every input, first and last byte; the previous one against the outputs
    assert call(m=out) == -2 and b"alias" in err() and call(m=out + n_img - 16) == -2 and call(m=out - n_mo + 16) == -2
    assert call(m=sn) == -2 and call(m=sn + n_st - 16) == -2 and call(m=sn - n_mo + 16) == -2
    assert call(m=img) == -2 and call(m=feat + n_feat - 16) == -2 and call(m=sp) == -2 and call(m=sp + n_st - 16) == -2
    assert call(m=mp) == -2 and call(m=mp + n_mo - 16) == -2 and call(m=mp - n_mo + 16) == -2 and b"d_moment_next" in err()
    assert call(q=sn) == -2 and call(q=sn + n_st - 16) == -2 and b"d_moment_prev" in err()
    assert call(q=out - n_mo + 16) == -2 and call(o=mp + n_mo - eb) == -2
    assert call(o=mn + n_mo - eb) == -2 and call(n=mn - n_st + 16) == -2
    # precedence: a null beats a bad parameter
    assert call(_t(gamma=9), m=0) == -1
    if not _has_gpu():
        rc = call()                                     # everything in order: only the device is missing
        assert rc not in (0, -1, -2, -5)
        assert call(cp=None, p=0, q=0) == rc            # the first frame is legal
        assert call(cp=None, p=0, q=0, o=sp, m=mp) == rc


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_noise_device_form_is_refused_without_a_device(lib, T):
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_history_noise_device_" + sfx)
    W, H = 10, 6
    n_st, n_mo, n_out = lib.rtw_temporal_state_bytes(W, H, eb), lib.rtw_history_moment_bytes(W, H, eb), W * H * eb
    st, mo, out = 0x300000, 0x600000, 0x800000
    err = lib.rtw_last_error
    vp = lambda x: C.c_void_p(x) if x else None

    def call(n=None, size=(W, H), s=st, m=mo, o=out, none=False):
        n = _n() if n is None else n
        return fn(None if none else C.byref(n), *size, vp(s), vp(m), vp(o), None)

    assert call(none=True) == -1 and b"null" in err()
    assert call(s=0) == -1 and call(m=0) == -1 and call(o=0) == -1
    for bad in BAD_N:
        assert call(_n(**bad)) == -2, bad
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    assert call(size=(2 ** 31 - 1, 2 ** 31 - 1)) == -5 and b"too large" in err()
    assert call(s=st + 8) == -2 and b"aligned" in err() and call(m=mo + 8) == -2 and call(o=out + 2) == -2 and b"aligned" in err()
    assert call(o=st) == -2 and b"alias" in err()
    assert call(o=st + n_st - eb) == -2 and call(o=st - n_out + eb) == -2 and call(o=mo) == -2 and call(o=mo + n_mo - eb) == -2 and call(o=mo - n_out + eb) == -2
    assert call(_n(radius=9), o=0) == -1                # a null beats a bad parameter
    if not _has_gpu():
        rc = call()
        assert rc not in (0, -1, -2, -5)
        assert call(o=out + eb) == rc                   # aligned to T is enough for the map
        for good in GOOD_N:
            assert call(_n(**good)) == rc, good


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_host_form_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_history_moments_" + sfx)
    W, H = 10, 6
    n, ns, nm = W * H, lib.rtw_temporal_state_bytes(W, H, eb) // eb, lib.rtw_history_moment_bytes(W, H, eb) // eb
    sizes = dict(i=n * 3, f=n * 8, o=n * 3, p=ns, nx=ns, q=nm, m=nm, r=n)
    buf = np.zeros(sum(sizes.values()) + 8, T)
    at, k = {}, 0
    for name, sz in sizes.items():
        at[name] = k
        k += sz
    view = lambda name, off=0: buf[at[name] + off:]
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    err = lib.rtw_last_error

    def call(t=None, nz=None, size=(W, H), c=cam, cp=cam, none=None, **over):
        t, nz = (_t() if t is None else t), (_n() if nz is None else nz)
        a = {name: view(name) for name in sizes}
        a.update(over)
        ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        ref = lambda x: None if x is None else C.byref(x)
        return fn(None if none == "t" else C.byref(t), None if none == "n" else C.byref(nz), ref(c), ref(cp), *size, ptr(a["i"]), ptr(a["f"]), ptr(a["p"]), ptr(a["q"]),
                  ptr(a["nx"]), ptr(a["m"]), ptr(a["o"]), ptr(a["r"]))

    assert call(none="t") == -1 and b"null" in err() and call(none="n") == -1
    for name in ("i", "f", "nx", "m", "o", "r"):
        assert call(**{name: None}) == -1, name
    assert call(c=None) == -1
    for bad in BAD_T:
        assert call(_t(**bad)) == -2, bad
    for bad in BAD_N:
        assert call(nz=_n(**bad)) == -2, bad
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    assert call(cp=None) == -2 and b"both" in err() and call(p=None) == -2 and b"both" in err()
    assert call(q=None) == -2 and b"moment_prev" in err() and call(cp=None, p=None) == -2 and b"moment_prev" in err()
    # every output against every other output and every input
    outs, ins = ("o", "nx", "m", "r"), ("i", "f", "p", "q")
    for a in outs:
        for b in outs + ins:
            if a != b:
                assert call(**{a: view(b)}) == -2 and b"alias" in err(), (a, b)
                assert call(**{a: view(b, sizes[b] - 1)}) == -2, (a, b)
    assert call(_t(gamma=9), o=None) == -1
    if not _has_gpu():
        assert call() not in (0, -1, -2, -5) and b"no HIP device" in err()
        assert call(cp=None, p=None, q=None) not in (0, -1, -2, -5)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_render_sequence_guided_is_refused_without_a_device(lib, rtw, T):
    """nulls (d among them: it is required), the step's, the map's and the filter's own checks, everything a batched feature render refuses,
    and DEMODULATE flags that differ"""
    from rtw_amd import _capi
    sfx = "f64" if T is np.float64 else "f32"
    fn = getattr(lib, "rtw_render_path_guided_" + sfx)
    S, keep = _capi.make_scene(rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T), T)
    N = 3
    cams = _capi.make_cameras([rtw.t_default_cam(elem_type=T)] * N, T)
    out = np.zeros(N * 96 * 54 * 3, T)
    dn = lambda **kw: _capi.Denoise(**dict(dict(levels=3, normal_power_log2=1, flags=1, gamma=1, device=-1, reserved=0, sigma_color=1.0, sigma_depth=0.1), **kw))
    err = lib.rtw_last_error

    def call(P, t=None, nz=None, d=None, scene=S, cm=cams, o=out, none=None, n=N):
        t, nz, d = (_t() if t is None else t), (_n() if nz is None else nz), (dn() if d is None else d)
        return fn(C.byref(scene) if scene is not None else None, cm, n, None, C.byref(P) if P is not None else None, None if none == "t" else C.byref(t),
                  None if none == "n" else C.byref(nz), None if none == "d" else C.byref(d), o.ctypes.data_as(C.c_void_p) if o is not None else None)

    P = _capi.make_params(96, 54, 4)
    assert call(None) == -1 and call(P, scene=None) == -1 and call(P, cm=None) == -1 and call(P, o=None) == -1
    assert call(P, none="t") == -1 and call(P, none="n") == -1 and call(P, none="d") == -1 and b"null" in err()
    for bad in BAD_T:
        assert call(P, _t(**bad)) == -2, bad
    for bad in BAD_N:
        assert call(P, nz=_n(**bad)) == -2, bad
    for bad in (dict(levels=0), dict(levels=9), dict(normal_power_log2=8), dict(flags=2), dict(gamma=2), dict(reserved=1), dict(device=-2), dict(sigma_color=0.0),
                dict(sigma_depth=float("nan"))):
        assert call(P, d=dn(**bad)) == -2, bad
    # the map is relative to the state's luminance: the two DEMODULATE flags agree
    assert call(P, _t(flags=0)) == -2 and b"DEMODULATE" in err()
    assert call(P, d=dn(flags=0)) == -2 and b"DEMODULATE" in err()
    # what a batched feature render refuses
    assert call(_capi.make_params(96, 54, 4, shard_index=0, shard_count=2)) == -2 and b"shard_count" in err()
    assert call(_capi.make_params(96, 54, 4, flags=_capi.FLAG_COMPACT_TILES)) == -2 and b"COMPACT_TILES" in err()
    assert call(_capi.make_params(96, 54, 4, flags=_capi.FLAG_RAY_POOL)) == -2 and b"RAY_POOL" in err()
    assert call(_capi.make_params(96, 54, 4, devices=[0, 1])) == -2 and b"n_devices" in err()
    assert call(_capi.make_params(0, 54, 4)) == -2 and call(_capi.make_params(96, 54, 0)) == -2
    assert call(_capi.make_params(2 ** 31 - 1, 2 ** 31 - 1, 4)) == -5
    assert call(P, n=0) == -2 and call(P, n=-2) == -2 and b"n_views" in err()
    assert call(None, _t(gamma=9)) == -1                        # a null beats a bad parameter
    if not _has_gpu():
        assert call(P) not in (0, -1, -2, -5) and b"no HIP device" in err()
        assert call(P, _t(flags=0), d=dn(flags=0)) not in (0, -1, -2, -5)       # both off is as good as both on
        assert call(P, n=1) not in (0, -1, -2, -5)
    del keep


def test_python_validation(rtw):
    T = np.float32
    img, feat = np.zeros((3, 5, 3), T), np.zeros((3, 5, 8), T)
    cam, cam64 = rtw.t_default_cam(elem_type=T), rtw.t_default_cam(elem_type=np.float64)
    n_state, n_mom = rtw.temporal_state_bytes(5, 3) // 4, rtw.temporal_moment_bytes(5, 3) // 4
    st, mo = np.zeros(n_state, T), np.zeros(n_mom, T)
    with pytest.raises(TypeError):
        rtw.temporal_step_moments(img, feat.astype(np.float64), cam)
    with pytest.raises(TypeError):
        rtw.temporal_step_moments(img, feat, cam64)
    with pytest.raises(ValueError):
        rtw.temporal_step_moments(img, feat[:, :4], cam)
    with pytest.raises(ValueError):
        rtw.temporal_step_moments(img[:0], feat[:0], cam)
    for kw in (dict(state=st), dict(moment=mo), dict(cam_prev=cam), dict(state=st, moment=mo), dict(state=st, cam_prev=cam), dict(moment=mo, cam_prev=cam)):
        with pytest.raises(ValueError, match="all"):
            rtw.temporal_step_moments(img, feat, cam, **kw)
    with pytest.raises(ValueError, match="state must be"):
        rtw.temporal_step_moments(img, feat, cam, state=np.zeros(n_state + 1, T), moment=mo, cam_prev=cam)
    with pytest.raises(ValueError, match="moment must be"):
        rtw.temporal_step_moments(img, feat, cam, state=st, moment=np.zeros(n_mom + 1, T), cam_prev=cam)
    with pytest.raises(ValueError, match="moment must be"):
        rtw.temporal_step_moments(img, feat, cam, state=st, moment=mo.astype(np.float64), cam_prev=cam)
    with pytest.raises(ValueError, match="keywords"):
        rtw.temporal_step_moments(img, feat, cam, noise=dict(levels=3))
    with pytest.raises(ValueError, match="all"):
        rtw.temporal_step_moments_into(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, cam, 5, 3, cam_prev=cam)
    with pytest.raises(ValueError, match="all"):
        rtw.temporal_step_moments_into(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, cam, 5, 3, d_state_prev_ptr=0x6000, cam_prev=cam)
    with pytest.raises(TypeError):
        rtw.temporal_step_moments_into(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, cam64, 5, 3)
    with pytest.raises(TypeError):
        rtw.temporal_noise_into(0x1000, 0x2000, 0x3000, 5, 3, levels=3)
    scene = rtw.scene_2_spheres(elem_type=T)
    with pytest.raises(ValueError, match="keywords"):
        rtw.render_sequence(scene, [cam, cam], 96, 4, guided=dict(sigma_color=1.0))
    with pytest.raises(ValueError, match="denoise"):
        rtw.render_sequence(scene, [cam, cam], 96, 4, guided=True, denoise=False)
    with pytest.raises(ValueError, match="demodulate"):
        rtw.render_sequence(scene, [cam, cam], 96, 4, guided=True, demodulate=False)
    with pytest.raises(ValueError, match="demodulate"):
        rtw.render_sequence(scene, [cam, cam], 96, 4, guided=True, denoise=dict(demodulate=False))
    tn = rtw.make_temporal_noise()
    assert (tn.radius, tn.normal_power_log2, tn.device, tuple(tn.reserved), tn.sigma_depth, tn.min_len) == (2, 1, -1, (0, 0, 0), 0.1, 4.0)
    tn = rtw.make_temporal_noise(3, 0, 0.5, 8, 2)
    assert (tn.radius, tn.normal_power_log2, tn.device, tn.sigma_depth, tn.min_len) == (3, 0, 2, 0.5, 8.0)
    assert "untuned" in rtw.make_temporal_noise.__doc__ and "untuned" in rtw.temporal_step_moments.__doc__ and "untuned" in rtw.temporal_noise_into.__doc__


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_moments_fail_loudly_without_gpu(rtw):
    from rtw_amd._capi import RtwError
    T = np.float32
    cam = rtw.t_default_cam(elem_type=T)
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.temporal_step_moments(np.zeros((3, 5, 3), T), np.zeros((3, 5, 8), T), cam)
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.render_sequence(rtw.scene_2_spheres(elem_type=T), [cam, cam], 96, 4, guided=True)
    with pytest.raises(ValueError, match="moments=True"):
        rtw.TemporalAccumulator.noise_into(type("A", (), dict(moments=False))(), 0x1000)


def test_c_sequence_guided_example_compiles_and_links(tmp_path):
    """examples/render_sequence_guided_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_sequence_guided_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "render_sequence_guided_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "2", "4"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr
