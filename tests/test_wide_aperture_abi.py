"""The wide-aperture stage, CPU only (include/rtw_hip.h rtw_wide_aperture_*, rtw_render_wide_aperture_*): the symbols are declared, listed and
exported and carry no substring by which an earlier ABI test pins its block's names, the struct and the workspace have the sizes the
header says, and every refusal of every new entry point is decided before any HIP call (the dummy device pointers below are never
dereferenced).  The refusals are the defocus stage's (tests/test_defocus_abi.py) with max_radius outside 1..32 in place of 1..8."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import defocus_ref as FO
import test_defocus_abi as DA
import wide_aperture_ref as WA
from conftest import ROOT
from test_temporal_noise_abi import BAD_SIZES, _has_gpu

SYMBOLS = ["rtw_wide_aperture_work_bytes", "rtw_wide_aperture_device_f32", "rtw_wide_aperture_device_f64", "rtw_wide_aperture_f32", "rtw_wide_aperture_f64",
           "rtw_render_wide_aperture_f32", "rtw_render_wide_aperture_f64"]
PY_NAMES = ["make_wide_aperture", "wide_aperture_work_bytes", "wide_aperture", "wide_aperture_into", "render_wide_aperture"]
#: the substrings by which the ABI tests of the other blocks pin their names (tests/test_defocus_abi.py's list and its own): no new name may carry one
PINNED = DA.PINNED + ["defocus"]
BAD_B = [b for b in DA.BAD_B if b != dict(max_radius=9)] + [dict(max_radius=33), dict(max_radius=2 ** 31 - 1)]
GOOD_B = DA.GOOD_B + [dict(max_radius=9), dict(max_radius=16), dict(max_radius=17), dict(max_radius=32)]
_bad_cameras = DA._bad_cameras


@pytest.fixture(scope="module")
def lib(rtw):
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def _b(**kw):
    from rtw_amd import _capi
    v = dict(max_radius=32, flags=0, gamma=1, device=-1, reserved=(0, 0), lens_radius=0.05, focus_dist=0.0)
    v.update(kw)
    v["reserved"] = (C.c_int32 * 2)(*v["reserved"])
    return _capi.WideAperture(**v)


def test_symbols_declared_exported_and_listed(lib, rtw):
    import inspect
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
        assert not any(s in name for s in PINNED), name
    assert sorted(n for n in declared if "wide_aperture" in n) == sorted(SYMBOLS)
    assert sorted(n for n in _capi.SYMBOLS if "wide_aperture" in n) == sorted(SYMBOLS)
    assert sorted(set(re.findall(r"\b(rtw_\w*wide_aperture\w*)\b", exported))) == sorted(SYMBOLS)
    assert lib.rtw_abi_version() == 4                    # additive: the ABI version stays
    for name in PY_NAMES:
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name
        assert not any(s in name for s in PINNED), name
    assert {"denoise", "wide_aperture"} <= set(inspect.signature(rtw.render_wide_aperture).parameters)
    assert C.sizeof(_capi.WideAperture) == 40 and re.search(r"\}\s*rtw_wide_aperture_t;\s*/\* 40 bytes \*/", header)
    assert [f[0] for f in _capi.WideAperture._fields_] == [f[0] for f in _capi.Defocus._fields_]
    assert re.search(r"#define\s+RTW_WIDE_APERTURE_MAX_RADIUS\s+32\b", header)
    block = header[header.index("Wide aperture: circles of confusion up to 32 px"):header.index("rtw_wide_aperture_work_bytes(int32_t")]
    for word in ("Left out on purpose", "batched views", "device lists", "the Julia shim", "bokeh shapes", "jittered taps", "ws > 0", "R_s <= Rm/s <= 8",
                 "each beginning on a multiple of four ELEMENTS", "keep refusing max_radius > 8"):
        assert word in block, word


def test_work_bytes(lib):
    """the witness's layout in bytes: a multiple of 16, monotone in the frame size, the defocus stage's for max_radius <= 8; bad sizes, element
    sizes and radii refused"""
    fn = lib.rtw_wide_aperture_work_bytes
    for eb in (4, 8):
        for mr in (1, 8, 9, 12, 16, 17, 24, 32):
            prev = 0
            for W, H in [(1, 1), (5, 3), (16, 16), (17, 16), (16, 17), (17, 33), (33, 17), (96, 54), (128, 72), (1920, 1080)]:
                n = fn(W, H, eb, mr)
                assert n == WA.work_elems(H, W, mr) * eb and n % 16 == 0 and n >= prev > -1, (W, H, eb, mr)
                assert (n == lib.rtw_defocus_work_bytes(W, H, eb)) == (mr <= 8)
                prev = n
            for W in range(1, 70):
                assert fn(W, 7, eb, mr) <= fn(W + 1, 7, eb, mr) and fn(7, W, eb, mr) <= fn(7, W + 1, eb, mr) and fn(W, 40, eb, mr) <= fn(W + 1, 40, eb, mr)
            for size, code in BAD_SIZES:
                assert fn(*size, eb, mr) == code, size
        for mr in (0, -1, 33, 2 ** 31 - 1):
            assert fn(10, 6, eb, mr) == -2 and b"max_radius" in lib.rtw_last_error()
    assert fn(10, 6, 2, 16) == -2 and fn(10, 6, 16, 16) == -2
    assert FO.work_elems(54, 96) * 4 == fn(96, 54, 4, 8)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_device_form_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_wide_aperture_device_" + sfx)
    W, H = 10, 6
    n_img, n_feat, n_work = W * H * 3 * eb, W * H * 8 * eb, lib.rtw_wide_aperture_work_bytes(W, H, eb, 32)
    img, feat, work, out = 0x100000, 0x200000, 0x400000, 0x500000       # never dereferenced
    assert n_work > lib.rtw_defocus_work_bytes(W, H, eb) and work + n_work < out
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    err = lib.rtw_last_error
    vp = lambda x: C.c_void_p(x) if x else None
    ref = lambda x: None if x is None else C.byref(x)

    def call(b="default", size=(W, H), c=cam, i=img, f=feat, w=work, o=out):
        return fn(ref(_b() if b == "default" else b), ref(c), *size, vp(i), vp(f), vp(w), vp(o), None)

    assert call(b=None) == -1 and b"null" in err()
    assert call(c=None) == -1 and call(i=0) == -1 and call(f=0) == -1 and call(w=0) == -1 and call(o=0) == -1
    for bad in BAD_B:
        assert call(_b(**bad)) == -2, bad
    assert call(_b(max_radius=33)) == -2 and b"1..32" in err()
    for name, bad in _bad_cameras(rtw, T):
        assert call(c=bad) == -2, name
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    assert call(f=feat + 8) == -2 and b"aligned" in err() and call(w=work + 8) == -2 and call(i=img + 2) == -2 and call(o=out + 1) == -2
    assert call(o=img) == -2 and b"alias" in err() and call(o=feat + n_feat - eb) == -2 and call(o=work + n_work - eb) == -2
    assert call(w=img) == -2 and b"alias" in err() and call(w=feat + 16) == -2 and call(w=out - n_work + 16) == -2 and call(w=img + n_img - 16) == -2
    # the workspace's size follows max_radius: behind the defocus stage's bytes a call with max_radius 8 owns nothing
    tail = work + lib.rtw_defocus_work_bytes(W, H, eb)
    assert call(_b(max_radius=9), o=tail) == -2 and b"alias" in err()
    assert call(_b(max_radius=33), o=0) == -1                 # precedence: a null beats a bad parameter
    if not _has_gpu():
        rc = call()                                     # everything in order: only the device is missing
        assert rc not in (0, -1, -2, -5)
        for good in GOOD_B:
            if good != dict(device=0):
                assert call(_b(**good)) == rc, good
        assert call(_b(max_radius=8), o=tail) == rc
        assert call(_b(focus_dist=3.0), c=dict(_bad_cameras(rtw, T))["focus0"]) == rc         # an override replaces the camera's own focus


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_host_form_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_wide_aperture_" + sfx)
    W, H = 10, 6
    n = W * H
    sizes = dict(i=n * 3, f=n * 8, o=n * 3)
    buf = np.zeros(sum(sizes.values()) + 8, T)
    at, k = {}, 0
    for name, sz in sizes.items():
        at[name] = buf.ctypes.data + k * eb
        k += sz
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    err = lib.rtw_last_error
    vp = lambda x: C.c_void_p(x) if x else None
    ref = lambda x: None if x is None else C.byref(x)

    def call(b="default", size=(W, H), c=cam, **ptr):
        a = dict(at)
        a.update(ptr)
        return fn(ref(_b() if b == "default" else b), ref(c), *size, vp(a["i"]), vp(a["f"]), vp(a["o"]))

    assert call(b=None) == -1 and call(c=None) == -1 and call(i=0) == -1 and call(f=0) == -1 and call(o=0) == -1
    for bad in BAD_B:
        assert call(_b(**bad)) == -2, bad
    for name, bad in _bad_cameras(rtw, T):
        assert call(c=bad) == -2, name
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    assert call(o=at["i"]) == -2 and b"alias" in err() and call(o=at["f"] + 16) == -2
    if not _has_gpu():
        rc = call()
        assert rc not in (0, -1, -2, -5)
        assert call(_b(max_radius=1, lens_radius=0.0)) == rc and call(_b(max_radius=9)) == rc


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_one_call_form_is_refused_without_a_device(lib, rtw, T):
    """rtw_render_wide_aperture_*: nulls (the filter alone is optional), the stage's own refusals -- lens_radius = -1 is the camera's own here
    and only here --, and everything the render, the feature pass and the filter refuse -- all before any HIP call"""
    from rtw_amd import _capi
    from rtw_amd.denoise import make_denoise
    sfx = "f64" if T is np.float64 else "f32"
    fn = getattr(lib, "rtw_render_wide_aperture_" + sfx)
    W, H = 10, 6
    S, keep = _capi.make_scene(rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T), T)
    cam = _capi.make_camera(rtw.t_cam1(elem_type=T), T)
    assert cam.lens_radius > 0
    out = np.zeros(W * H * 3, T)
    err = lib.rtw_last_error
    P = lambda **kw: _capi.make_params(kw.pop("w", W), kw.pop("h", H), kw.pop("spp", 2), **kw)
    ref = lambda x: None if x is None else C.byref(x)

    def call(p="default", d=None, b="default", s=S, c=cam, o=out.ctypes.data):
        return fn(ref(s), ref(c), ref(P() if p == "default" else p), ref(d), ref(_b() if b == "default" else b), C.c_void_p(o) if o else None)

    assert call(p=None) == -1 and b"null" in err() and call(b=None) == -1 and call(s=None) == -1 and call(c=None) == -1 and call(o=0) == -1
    for bad in BAD_B:
        if bad != dict(lens_radius=-1.0):
            assert call(b=_b(**bad)) == -2, bad
    bad_cam = _capi.make_camera(rtw.t_cam1(elem_type=T), T)
    bad_cam.lens_radius = -0.25
    assert call(b=_b(lens_radius=-1.0), c=bad_cam) == -2          # the camera's own, and that is negative
    for name, bad in _bad_cameras(rtw, T):
        assert call(c=bad) == -2, name
    for size, code in BAD_SIZES:
        assert call(P(w=size[0], h=size[1])) == code, size
    assert call(P(spp=0)) == -2 and call(P(flags=_capi.FLAG_COMPACT_TILES)) == -2 and call(d=make_denoise(levels=0)) == -2
    bad_scene, keep2 = _capi.make_scene(rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T), T)
    bad_scene.n = -1
    assert call(s=bad_scene) == -2 and b"sphere count" in err()
    if not _has_gpu():
        rc = call()
        assert rc not in (0, -1, -2, -4, -5)                  # everything in order: only the device is missing
        assert call(b=_b(lens_radius=-1.0)) == rc and call(d=make_denoise()) == rc and call(b=_b(focus_dist=7.0, max_radius=3)) == rc and call(b=_b(max_radius=12)) == rc
    del keep, keep2


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_one_call_form_refuses_a_radius_beyond_its_own_bound_and_names_no_view(lib, rtw, T):
    """rtw_render_wide_aperture_* with max_radius = 33: -2 with this stage's bound, 1..32; a single call names no view"""
    from rtw_amd import _capi
    fn = getattr(lib, "rtw_render_wide_aperture_" + ("f64" if T is np.float64 else "f32"))
    W, H = 10, 6
    S, keep = _capi.make_scene(rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T), T)
    cam = _capi.make_camera(rtw.t_cam1(elem_type=T), T)
    out = np.zeros(W * H * 3, T)
    assert fn(C.byref(S), C.byref(cam), C.byref(_capi.make_params(W, H, 2)), None, C.byref(_b(max_radius=33)), out.ctypes.data_as(C.c_void_p)) == -2
    err = lib.rtw_last_error()
    assert b"1..32" in err and b"view" not in err, err
    del keep


def test_the_python_layer_checks_its_arguments(rtw):
    T = np.float32
    cam = rtw.t_default_cam(elem_type=T)
    img, feat = np.zeros((6, 10, 3), T), np.zeros((6, 10, 8), T)
    with pytest.raises(TypeError):
        rtw.wide_aperture(img, feat.astype(np.float64), cam, lens_radius=0.1)
    with pytest.raises(ValueError):
        rtw.wide_aperture(img, feat[:, :5], cam, lens_radius=0.1)
    with pytest.raises(TypeError):
        rtw.wide_aperture(img, feat, None, lens_radius=0.1)
    with pytest.raises(TypeError):
        rtw.wide_aperture(img, feat, rtw.t_default_cam(elem_type=np.float64), lens_radius=0.1)
    with pytest.raises(Exception) as e:
        rtw.wide_aperture(img, feat, cam, lens_radius=0.1, max_radius=33)
    assert "max_radius" in str(e.value)
    with pytest.raises(Exception) as e:
        rtw.wide_aperture_work_bytes(96, 54, max_radius=0)
    assert "max_radius" in str(e.value)
    with pytest.raises(ValueError):
        rtw.render_wide_aperture(rtw.scene_2_spheres(elem_type=T), cam, 16, 1, wide_aperture=dict(radius=3))
    with pytest.raises(ValueError):
        rtw.render_wide_aperture(rtw.scene_2_spheres(elem_type=T), cam, 16, 1, denoise=dict(taps=3))
    assert rtw.wide_aperture_work_bytes(96, 54) == WA.work_elems(54, 96, 32) * 4 and rtw.wide_aperture_work_bytes(96, 54, np.float64, 16) == WA.work_elems(54, 96, 16) * 8
    assert rtw.wide_aperture_work_bytes(96, 54, max_radius=8) == rtw.defocus_work_bytes(96, 54)
    assert rtw.make_wide_aperture(0.1).max_radius == 32


def test_c_example_compiles_and_links(tmp_path):
    """examples/render_wide_aperture_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_wide_aperture_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "render_wide_aperture_c.c"),
                        "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "2"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr
