"""The defocus stage, CPU only (include/rtw_hip.h rtw_defocus_*, rtw_render_defocused_*): the symbols are declared, listed and exported, the
struct and the workspace have the sizes the header says, and every refusal of every new entry point is decided before any HIP call (the
dummy device pointers below are never dereferenced)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import defocus_ref as FO
from conftest import ROOT
from test_temporal_noise_abi import BAD_SIZES, _has_gpu

DEFOCUS_SYMBOLS = ["rtw_defocus_work_bytes", "rtw_defocus_device_f32", "rtw_defocus_device_f64", "rtw_defocus_f32", "rtw_defocus_f64", "rtw_render_defocused_f32",
                   "rtw_render_defocused_f64"]
PY_NAMES = ["make_defocus", "defocus_work_bytes", "defocus", "defocus_into", "render_defocused"]
#: the substrings by which the ABI tests of the other blocks pin their names: no new name may carry one
PINNED = ["blur", "motion", "animat", "denois", "present", "upsampl", "temporal", "sequence", "history", "path_guided", "clamped", "reproject", "render_paths"]
BAD_B = [dict(max_radius=0), dict(max_radius=9), dict(max_radius=-1), dict(flags=1), dict(flags=-1), dict(gamma=2), dict(gamma=-1), dict(device=-2), dict(reserved=(1, 0)),
         dict(reserved=(0, -1)), dict(lens_radius=-0.5), dict(lens_radius=-1.0), dict(lens_radius=float("nan")), dict(lens_radius=float("inf")), dict(focus_dist=-1.0),
         dict(focus_dist=float("inf")), dict(focus_dist=float("nan"))]
GOOD_B = [dict(max_radius=1), dict(max_radius=8), dict(lens_radius=0.0), dict(lens_radius=1e6), dict(focus_dist=1e-9), dict(focus_dist=1e9), dict(gamma=0), dict(device=0)]


@pytest.fixture(scope="module")
def lib(rtw):
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def _b(**kw):
    from rtw_amd import _capi
    v = dict(max_radius=8, flags=0, gamma=1, device=-1, reserved=(0, 0), lens_radius=0.05, focus_dist=0.0)
    v.update(kw)
    v["reserved"] = (C.c_int32 * 2)(*v["reserved"])
    return _capi.Defocus(**v)


def _bad_cameras(rtw, T):
    """cameras the stage refuses: a horizontal vector of length 0 or infinity, a focus plane at or behind the eye, a focus that is not finite"""
    from rtw_amd import _capi
    out = []
    for edit in ("hor0", "hor_inf", "focus0", "focus_neg", "focus_nan"):
        cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
        if edit == "hor0":
            cam.horizontal[0] = cam.horizontal[1] = cam.horizontal[2] = 0
        elif edit == "hor_inf":
            cam.horizontal[0] = float("inf")
        elif edit == "focus0":
            for k in range(3):
                cam.lower_left_corner[k] = cam.origin[k]
        elif edit == "focus_neg":
            for k in range(3):
                cam.lower_left_corner[k] = cam.origin[k] + cam.w[k]
        else:
            cam.lower_left_corner[2] = float("nan")
        out.append((edit, cam))
    return out


def test_symbols_declared_exported_and_listed(lib, rtw):
    import inspect
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in DEFOCUS_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
        assert not any(s in name for s in PINNED), name
    assert sorted(n for n in declared if "defocus" in n) == sorted(DEFOCUS_SYMBOLS)
    assert sorted(n for n in _capi.SYMBOLS if "defocus" in n) == sorted(DEFOCUS_SYMBOLS)
    assert sorted(set(re.findall(r"\b(rtw_\w*defocus\w*)\b", exported))) == sorted(DEFOCUS_SYMBOLS)
    assert lib.rtw_abi_version() == 4                    # additive: the ABI version stays
    for name in PY_NAMES:
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name
    assert {"denoise", "defocus"} <= set(inspect.signature(rtw.render_defocused).parameters)
    assert C.sizeof(_capi.Defocus) == 40 and re.search(r"\}\s*rtw_defocus_t;\s*/\* 40 bytes \*/", header)
    assert re.search(r"#define\s+RTW_DEFOCUS_TILE\s+16\b", header) and re.search(r"#define\s+RTW_DEFOCUS_MAX_RADIUS\s+8\b", header)
    block = header[header.index("Depth of field: a gather on a finished pinhole frame"):header.index("rtw_defocus_work_bytes(int32_t")]
    for word in ("Left out on purpose", "batched views", "device lists", "the Julia shim", "radii beyond 8 px", "bokeh shapes", "jittered taps", "any reduction tree",
                 "no arithmetic is done on an infinity", "the camera's own"):
        assert word in block, word


def test_work_bytes(lib):
    """the CoC plane of 4-element slots and one element per tile, rounded up to four: a multiple of 16, monotone in the size, the witness's count;
    bad sizes refused"""
    fn = lib.rtw_defocus_work_bytes
    for eb in (4, 8):
        prev = 0
        for W, H in [(1, 1), (5, 3), (16, 16), (17, 16), (16, 17), (17, 33), (33, 17), (96, 54), (128, 72), (1920, 1080)]:
            n = fn(W, H, eb)
            assert n == FO.work_elems(H, W) * eb and n % 16 == 0 and n >= prev > -1, (W, H, eb)
            prev = n
        for W in range(1, 70):
            assert fn(W, 7, eb) <= fn(W + 1, 7, eb) and fn(7, W, eb) <= fn(7, W + 1, eb) and fn(W, 40, eb) <= fn(W + 1, 40, eb)
        for size, code in BAD_SIZES:
            assert fn(*size, eb) == code, size
    assert fn(10, 6, 2) == -2 and fn(10, 6, 16) == -2


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_device_form_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_defocus_device_" + sfx)
    W, H = 10, 6
    n_img, n_feat, n_work = W * H * 3 * eb, W * H * 8 * eb, lib.rtw_defocus_work_bytes(W, H, eb)
    img, feat, work, out = 0x100000, 0x200000, 0x400000, 0x500000       # never dereferenced
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
    for name, bad in _bad_cameras(rtw, T):
        assert call(c=bad) == -2, name
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    assert call(f=feat + 8) == -2 and b"aligned" in err() and call(w=work + 8) == -2 and call(i=img + 2) == -2 and call(o=out + 1) == -2
    assert call(o=img) == -2 and b"alias" in err() and call(o=feat + n_feat - eb) == -2 and call(o=work + n_work - eb) == -2
    assert call(w=img) == -2 and b"alias" in err() and call(w=feat + 16) == -2 and call(w=out - n_work + 16) == -2 and call(w=img + n_img - 16) == -2
    assert call(_b(max_radius=9), o=0) == -1                  # precedence: a null beats a bad parameter
    if not _has_gpu():
        rc = call()                                     # everything in order: only the device is missing
        assert rc not in (0, -1, -2, -5)
        for good in GOOD_B:
            if good != dict(device=0):
                assert call(_b(**good)) == rc, good
        assert call(_b(focus_dist=3.0), c=dict(_bad_cameras(rtw, T))["focus0"]) == rc         # an override replaces the camera's own focus


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_host_form_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_defocus_" + sfx)
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
        assert call(_b(max_radius=1, lens_radius=0.0)) == rc


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_one_call_form_is_refused_without_a_device(lib, rtw, T):
    """rtw_render_defocused_*: nulls (the filter alone is optional), the stage's own refusals -- lens_radius = -1 is the camera's own here and
    only here --, and everything the render, the feature pass and the filter refuse -- all before any HIP call"""
    from rtw_amd import _capi
    from rtw_amd.denoise import make_denoise
    sfx = "f64" if T is np.float64 else "f32"
    fn = getattr(lib, "rtw_render_defocused_" + sfx)
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
        assert call(b=_b(lens_radius=-1.0)) == rc and call(d=make_denoise()) == rc and call(b=_b(focus_dist=7.0, max_radius=3)) == rc
    del keep, keep2


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_one_call_form_refuses_a_radius_beyond_its_own_bound_and_names_no_view(lib, rtw, T):
    """rtw_render_defocused_* with max_radius = 9: -2 with the defocus stage's bound, 1..8, not the wide-aperture stage's; a single call
    names no view"""
    from rtw_amd import _capi
    fn = getattr(lib, "rtw_render_defocused_" + ("f64" if T is np.float64 else "f32"))
    W, H = 10, 6
    S, keep = _capi.make_scene(rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T), T)
    cam = _capi.make_camera(rtw.t_cam1(elem_type=T), T)
    out = np.zeros(W * H * 3, T)
    assert fn(C.byref(S), C.byref(cam), C.byref(_capi.make_params(W, H, 2)), None, C.byref(_b(max_radius=9)), out.ctypes.data_as(C.c_void_p)) == -2
    err = lib.rtw_last_error()
    assert b"1..8" in err and b"view" not in err, err
    del keep


def test_the_python_layer_checks_its_arguments(rtw):
    T = np.float32
    cam = rtw.t_default_cam(elem_type=T)
    img, feat = np.zeros((6, 10, 3), T), np.zeros((6, 10, 8), T)
    with pytest.raises(TypeError):
        rtw.defocus(img, feat.astype(np.float64), cam, lens_radius=0.1)
    with pytest.raises(ValueError):
        rtw.defocus(img, feat[:, :5], cam, lens_radius=0.1)
    with pytest.raises(TypeError):
        rtw.defocus(img, feat, None, lens_radius=0.1)
    with pytest.raises(TypeError):
        rtw.defocus(img, feat, rtw.t_default_cam(elem_type=np.float64), lens_radius=0.1)
    with pytest.raises(Exception) as e:
        rtw.defocus(img, feat, cam, lens_radius=0.1, max_radius=9)
    assert "max_radius" in str(e.value)
    with pytest.raises(ValueError):
        rtw.render_defocused(rtw.scene_2_spheres(elem_type=T), cam, 16, 1, defocus=dict(radius=3))
    with pytest.raises(ValueError):
        rtw.render_defocused(rtw.scene_2_spheres(elem_type=T), cam, 16, 1, denoise=dict(taps=3))
    assert rtw.defocus_work_bytes(96, 54) == FO.work_elems(54, 96) * 4 and rtw.defocus_work_bytes(96, 54, np.float64) == FO.work_elems(54, 96) * 8


def test_c_example_compiles_and_links(tmp_path):
    """examples/render_defocused_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_defocused_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "render_defocused_c.c"),
                        "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "2"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr
