"""The temporal clamp, CPU only (include/rtw_hip.h rtw_clamped_step_*, rtw_render_path_clamped_*): the symbols are declared, listed and
exported, the struct has its 32 bytes, and every refusal of every new entry point is decided before any HIP call (the dummy device pointers
below are never dereferenced)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_temporal_noise_abi import BAD_N, BAD_SIZES, BAD_T, _has_gpu, _n, _t

CLAMP_SYMBOLS = ["rtw_clamped_step_device_f32", "rtw_clamped_step_device_f64", "rtw_clamped_step_f32", "rtw_clamped_step_f64",
                 "rtw_render_path_clamped_f32", "rtw_render_path_clamped_f64"]
BAD_C = [dict(radius=0), dict(radius=4), dict(radius=-1), dict(flags=2), dict(flags=-1), dict(flags=3), dict(reserved=(1, 0)), dict(reserved=(0, -1)),
         dict(sigma=-0.5), dict(sigma=float("inf")), dict(sigma=float("nan")), dict(len_scale=-0.25), dict(len_scale=1.5), dict(len_scale=float("nan")),
         dict(len_scale=float("inf"))]
GOOD_C = [dict(radius=1), dict(radius=3), dict(flags=1), dict(sigma=0.0), dict(sigma=1e6), dict(len_scale=0.0), dict(len_scale=1.0)]


@pytest.fixture(scope="module")
def lib(rtw):
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def _c(**kw):
    from rtw_amd import _capi
    v = dict(radius=1, flags=0, reserved=(0, 0), sigma=1.0, len_scale=1.0)
    v.update(kw)
    v["reserved"] = (C.c_int32 * 2)(*v["reserved"])
    return _capi.TemporalClamp(**v)


def test_symbols_declared_exported_and_listed(lib, rtw):
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in CLAMP_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert sorted(n for n in declared if "clamped" in n) == sorted(CLAMP_SYMBOLS)
    assert lib.rtw_abi_version() == 4                    # additive: the ABI version stays
    assert "rtw_temporal_clamp_t" in header and re.search(r"#define\s+RTW_CLAMP_GUIDES\s+1\b", header)
    for name in ("make_temporal_clamp", "temporal_step_clamped", "temporal_step_clamped_into"):
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name
    assert "UNTUNED" in header[header.index("Temporal clamp"):]


def test_the_struct_has_32_bytes(tmp_path):
    from rtw_amd import _capi
    S = _capi.TemporalClamp
    assert C.sizeof(S) == 32
    assert S.radius.offset == 0 and S.flags.offset == 4 and S.reserved.offset == 8 and S.sigma.offset == 16 and S.len_scale.offset == 24
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtw_hip.h"\n'
                   'int main(void) { printf("%d %d %d %d %d %d %d\\n", (int)sizeof(rtw_temporal_clamp_t), (int)offsetof(rtw_temporal_clamp_t, flags), '
                   '(int)offsetof(rtw_temporal_clamp_t, reserved), (int)offsetof(rtw_temporal_clamp_t, sigma), (int)offsetof(rtw_temporal_clamp_t, len_scale), '
                   '(int)sizeof(rtw_temporal_t), (int)sizeof(rtw_temporal_noise_t)); return 0; }\n')
    exe = str(tmp_path / "size")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([exe], capture_output=True, text=True).stdout.split() == ["32", "4", "8", "16", "24", "48", "40"]


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_device_form_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_clamped_step_device_" + sfx)
    W, H = 10, 6
    n_img, n_st, n_mo = W * H * 3 * eb, lib.rtw_temporal_state_bytes(W, H, eb), lib.rtw_history_moment_bytes(W, H, eb)
    img, feat, sp, sn, out, mp, mn = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000       # never dereferenced
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    err = lib.rtw_last_error
    vp = lambda x: C.c_void_p(x) if x else None

    def call(t=None, k=None, size=(W, H), c=cam, cp=cam, i=img, f=feat, p=sp, q=mp, n=sn, m=mn, o=out, none=None):
        t, k = (_t() if t is None else t), (_c() if k is None else k)
        ref = lambda x: None if x is None else C.byref(x)
        return fn(None if none == "t" else C.byref(t), None if none == "c" else C.byref(k), ref(c), ref(cp), *size, vp(i), vp(f), vp(p), vp(q), vp(n), vp(m), vp(o), None)

    assert call(none="c") == -1 and b"null" in err() and call(none="t") == -1
    assert call(c=None) == -1 and call(i=0) == -1 and call(f=0) == -1 and call(n=0) == -1 and call(o=0) == -1
    assert call(m=0) == -1                              # a previous moment plane without a next one
    for bad in BAD_C:
        assert call(k=_c(**bad)) == -2 and b"clamp" in err(), bad
        assert call(k=_c(**bad), q=0, m=0) == -2, bad   # ... and without moments
    for bad in BAD_T:
        assert call(_t(**bad)) == -2, bad
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    # the rules of the underlying calls: the first frame's nulls come together, alignment, aliasing
    assert call(cp=None) == -2 and b"both" in err() and call(p=0) == -2 and b"both" in err()
    assert call(q=0) == -2 and b"d_moment_prev" in err() and call(cp=None, p=0) == -2 and b"d_moment_prev" in err()
    assert call(q=0, m=0, cp=None) == -2 and b"both" in err()
    assert call(f=feat + 8) == -2 and call(p=sp + 8) == -2 and call(n=sn + 8) == -2 and b"aligned" in err()
    assert call(q=mp + 8) == -2 and b"moment" in err() and call(m=mn + 4) == -2 and call(i=img + 2) == -2 and call(o=out + 2) == -2
    assert call(o=sn) == -2 and b"alias" in err() and call(o=img + n_img - eb) == -2 and call(n=sp) == -2
    assert call(m=out) == -2 and call(m=sn + n_st - 16) == -2 and call(m=mp) == -2 and call(q=sn) == -2 and call(o=mn + n_mo - eb) == -2
    assert call(q=0, m=0, o=sn) == -2 and b"alias" in err()
    # precedence: a null beats a bad parameter
    assert call(k=_c(radius=9), o=0) == -1 and call(_t(gamma=9), none="c") == -1
    if not _has_gpu():
        rc = call()                                     # everything in order: only the device is missing
        assert rc not in (0, -1, -2, -5)
        assert call(q=0, m=0) == rc                     # no moments
        assert call(cp=None, p=0, q=0) == rc and call(cp=None, p=0, q=0, m=0) == rc          # the first frame is legal, with and without moments
        for good in GOOD_C:
            assert call(k=_c(**good)) == rc, good


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_host_form_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_clamped_step_" + sfx)
    W, H = 10, 6
    n, ns, nm = W * H, lib.rtw_temporal_state_bytes(W, H, eb) // eb, lib.rtw_history_moment_bytes(W, H, eb) // eb
    sizes = dict(i=n * 3, f=n * 8, o=n * 3, p=ns, nx=ns, q=nm, m=nm)
    buf = np.zeros(sum(sizes.values()) + 8, T)
    at, k = {}, 0
    for name, sz in sizes.items():
        at[name] = k
        k += sz
    view = lambda name, off=0: buf[at[name] + off:]
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    err = lib.rtw_last_error

    def call(t=None, k=None, size=(W, H), c=cam, cp=cam, none=None, **over):
        t, k = (_t() if t is None else t), (_c() if k is None else k)
        a = {name: view(name) for name in sizes}
        a.update(over)
        ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        ref = lambda x: None if x is None else C.byref(x)
        return fn(None if none == "t" else C.byref(t), None if none == "c" else C.byref(k), ref(c), ref(cp), *size, ptr(a["i"]), ptr(a["f"]), ptr(a["p"]), ptr(a["q"]),
                  ptr(a["nx"]), ptr(a["m"]), ptr(a["o"]))

    assert call(none="c") == -1 and b"null" in err() and call(none="t") == -1
    for name in ("i", "f", "nx", "o", "m"):
        assert call(**{name: None}) == -1, name
    assert call(c=None) == -1
    for bad in BAD_C:
        assert call(k=_c(**bad)) == -2 and b"clamp" in err(), bad
    for bad in BAD_T:
        assert call(_t(**bad)) == -2, bad
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    assert call(cp=None) == -2 and b"both" in err() and call(p=None) == -2 and b"both" in err()
    assert call(q=None) == -2 and b"moment_prev" in err() and call(cp=None, p=None) == -2 and b"moment_prev" in err()
    outs, ins = ("o", "nx", "m"), ("i", "f", "p", "q")
    for a in outs:
        for b in outs + ins:
            if a != b:
                assert call(**{a: view(b)}) == -2 and b"alias" in err(), (a, b)
                assert call(**{a: view(b, sizes[b] - 1)}) == -2, (a, b)
    assert call(k=_c(radius=9), o=None) == -1
    if not _has_gpu():
        assert call() not in (0, -1, -2, -5) and b"no HIP device" in err()
        assert call(q=None, m=None) not in (0, -1, -2, -5)
        assert call(cp=None, p=None, q=None) not in (0, -1, -2, -5) and call(cp=None, p=None, q=None, m=None) not in (0, -1, -2, -5)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_render_path_clamped_is_refused_without_a_device(lib, rtw, T):
    """nulls (c among them; n and d are optional), n without d, the clamp's, the step's, the map's and the filter's own checks, and everything a
    batched feature render refuses -- with the underlying call's code"""
    from rtw_amd import _capi
    sfx = "f64" if T is np.float64 else "f32"
    fn = getattr(lib, "rtw_render_path_clamped_" + sfx)
    S, keep = _capi.make_scene(rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T), T)
    N = 3
    cams = _capi.make_cameras([rtw.t_default_cam(elem_type=T)] * N, T)
    out = np.zeros(N * 96 * 54 * 3, T)
    dn = lambda **kw: _capi.Denoise(**dict(dict(levels=3, normal_power_log2=1, flags=1, gamma=1, device=-1, reserved=0, sigma_color=1.0, sigma_depth=0.1), **kw))
    err = lib.rtw_last_error

    def call(P, t=None, k=None, nz=None, d=None, scene=S, cm=cams, o=out, none=(), n=N):
        t, k, nz, d = (_t() if t is None else t), (_c() if k is None else k), (_n() if nz is None else nz), (dn() if d is None else d)
        return fn(C.byref(scene) if scene is not None else None, cm, n, None, C.byref(P) if P is not None else None, None if "t" in none else C.byref(t),
                  None if "c" in none else C.byref(k), None if "n" in none else C.byref(nz), None if "d" in none else C.byref(d),
                  o.ctypes.data_as(C.c_void_p) if o is not None else None)

    P = _capi.make_params(96, 54, 4)
    for form in ((), ("n",), ("n", "d")):               # guided, the plain filter, no filter
        assert call(None, none=form) == -1 and call(P, scene=None, none=form) == -1 and call(P, cm=None, none=form) == -1 and call(P, o=None, none=form) == -1
        assert call(P, none=form + ("t",)) == -1 and call(P, none=form + ("c",)) == -1 and b"null" in err()
        for bad in BAD_C:
            assert call(P, k=_c(**bad), none=form) == -2 and b"clamp" in err(), (form, bad)
        for bad in BAD_T:
            assert call(P, _t(**bad), none=form) == -2, (form, bad)
        assert call(_capi.make_params(96, 54, 4, shard_index=0, shard_count=2), none=form) == -2 and b"shard_count" in err()
        assert call(_capi.make_params(96, 54, 4, devices=[0, 1]), none=form) == -2 and b"n_devices" in err()
        assert call(_capi.make_params(0, 54, 4), none=form) == -2 and call(_capi.make_params(2 ** 31 - 1, 2 ** 31 - 1, 4), none=form) == -5
        assert call(P, n=0, none=form) == -2 and b"n_views" in err()
        assert call(None, k=_c(radius=9), none=form) == -1          # a null beats a bad parameter
    assert call(P, none=("d",)) == -2 and b"d is required" in err()         # n without d
    for bad in BAD_N:
        assert call(P, nz=_n(**bad)) == -2, bad
    for bad in (dict(levels=0), dict(flags=2), dict(sigma_color=0.0)):
        assert call(P, d=dn(**bad)) == -2 and call(P, d=dn(**bad), none=("n",)) == -2, bad
    assert call(P, _t(flags=0)) == -2 and b"DEMODULATE" in err()            # the guided form's own rule
    if not _has_gpu():
        for form in ((), ("n",), ("n", "d")):
            assert call(P, none=form) not in (0, -1, -2, -5) and b"no HIP device" in err()
            for good in GOOD_C:
                assert call(P, k=_c(**good), none=form) not in (0, -1, -2, -5), good
    del keep


def test_python_validation(rtw):
    T = np.float32
    img, feat = np.zeros((3, 5, 3), T), np.zeros((3, 5, 8), T)
    cam, cam64 = rtw.t_default_cam(elem_type=T), rtw.t_default_cam(elem_type=np.float64)
    n_state, n_mom = rtw.temporal_state_bytes(5, 3) // 4, rtw.temporal_moment_bytes(5, 3) // 4
    st, mo = np.zeros(n_state, T), np.zeros(n_mom, T)
    with pytest.raises(TypeError):
        rtw.temporal_step_clamped(img, feat.astype(np.float64), cam)
    with pytest.raises(TypeError):
        rtw.temporal_step_clamped(img, feat, cam64)
    with pytest.raises(ValueError):
        rtw.temporal_step_clamped(img, feat[:, :4], cam)
    with pytest.raises(ValueError, match="clamp"):
        rtw.temporal_step_clamped(img, feat, cam, clamp=None)
    with pytest.raises(ValueError, match="keywords"):
        rtw.temporal_step_clamped(img, feat, cam, clamp=dict(levels=3))
    for kw in (dict(state=st), dict(cam_prev=cam), dict(moment=mo), dict(state=st, moment=mo), dict(moment=mo, cam_prev=cam), dict(state=st, cam_prev=cam, moments=True)):
        with pytest.raises(ValueError, match="all"):
            rtw.temporal_step_clamped(img, feat, cam, **kw)
    with pytest.raises(ValueError, match="state must be"):
        rtw.temporal_step_clamped(img, feat, cam, state=np.zeros(n_state + 1, T), cam_prev=cam)
    with pytest.raises(ValueError, match="moment must be"):
        rtw.temporal_step_clamped(img, feat, cam, state=st, moment=np.zeros(n_mom + 1, T), cam_prev=cam)
    with pytest.raises(ValueError, match="all"):
        rtw.temporal_step_clamped_into(0x1000, 0x2000, 0x3000, 0x4000, cam, 5, 3, cam_prev=cam)
    with pytest.raises(ValueError, match="all"):
        rtw.temporal_step_clamped_into(0x1000, 0x2000, 0x3000, 0x4000, cam, 5, 3, d_state_prev_ptr=0x6000, cam_prev=cam, d_moment_next_ptr=0x7000)
    with pytest.raises(ValueError, match="clamp"):
        rtw.temporal_step_clamped_into(0x1000, 0x2000, 0x3000, 0x4000, cam, 5, 3, clamp=False)
    with pytest.raises(ValueError, match="keywords"):
        rtw.TemporalAccumulator.__init__(type("A", (), {})(), 5, 3, clamp=dict(sigma_color=1.0))
    scene = rtw.scene_2_spheres(elem_type=T)
    with pytest.raises(ValueError, match="keywords"):
        rtw.render_sequence(scene, [cam, cam], 96, 4, clamp=dict(min_len=2.0))
    tc = rtw.make_temporal_clamp()
    assert (tc.radius, tc.flags, tuple(tc.reserved), tc.sigma, tc.len_scale) == (1, 0, (0, 0), 1.0, 1.0)
    tc = rtw.make_temporal_clamp(3, True, 0.5, 0.25)
    assert (tc.radius, tc.flags, tc.sigma, tc.len_scale) == (3, 1, 0.5, 0.25)
    assert all("untuned" in f.__doc__ for f in (rtw.make_temporal_clamp, rtw.temporal_step_clamped, rtw.temporal_step_clamped_into, rtw.render_sequence))


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_the_clamped_calls_fail_loudly_without_gpu(rtw):
    from rtw_amd._capi import RtwError
    T = np.float32
    cam = rtw.t_default_cam(elem_type=T)
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.temporal_step_clamped(np.zeros((3, 5, 3), T), np.zeros((3, 5, 8), T), cam)
    for kw in (dict(), dict(denoise=True), dict(guided=True)):
        with pytest.raises(RtwError, match="no HIP device"):
            rtw.render_sequence(rtw.scene_2_spheres(elem_type=T), [cam, cam], 96, 4, clamp=True, **kw)


def test_c_sequence_clamped_example_compiles_and_links(tmp_path):
    """examples/render_sequence_clamped_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_sequence_clamped_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "render_sequence_clamped_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "2", "4"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr
