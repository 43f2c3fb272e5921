"""The batched lens stages, CPU only (include/rtw_hip.h rtw_lens_table_*, rtw_lens_batch_*, rtw_render_lens_batch_*): the ten names are
declared, listed and exported and carry no substring by which an earlier ABI test pins its block's names; the workspace is n_views single
ones; the lens table equals its restatement (tests/lens_batch_ref.py) on the bits; and every refusal of every new entry point is decided
before any HIP call, with its code and a message (the dummy device pointers below are never dereferenced)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import defocus_ref as FO
import lens_batch_ref as LB
import test_defocus_abi as DA
import test_wide_aperture_abi as WAA
from conftest import ROOT
from test_temporal_noise_abi import BAD_SIZES, _has_gpu

SYMBOLS = ["rtw_lens_table_bytes", "rtw_lens_table_f32", "rtw_lens_table_f64", "rtw_lens_batch_work_bytes", "rtw_lens_batch_device_f32", "rtw_lens_batch_device_f64",
           "rtw_lens_batch_f32", "rtw_lens_batch_f64", "rtw_render_lens_batch_f32", "rtw_render_lens_batch_f64"]
PY_NAMES = ["lens_table", "wide_aperture_batch_work_bytes", "wide_aperture_batch", "wide_aperture_batch_into", "focus_bracket", "render_wide_aperture_batch"]
PINNED = WAA.PINNED + ["wide_aperture"]
#: what the device form reads of `b`: max_radius, gamma, device, flags, reserved -- the lens lives in the table
BAD_B_DEVICE = [b for b in WAA.BAD_B if not ({"lens_radius", "focus_dist"} & set(b))]
BAD_LENS = [-0.5, float("nan"), float("inf")]
BAD_FOCUS = [-1.0, float("inf"), float("nan")]
_b = WAA._b
_bad_cameras = DA._bad_cameras


@pytest.fixture(scope="module")
def lib(rtw):
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def _dbl(values):
    return None if values is None else (C.c_double * len(values))(*values)


def _cams(rtw, T, n, edit=None):
    """n copies of the default camera as a ctypes array; edit = (v, camera struct): view v replaced"""
    from rtw_amd import _capi
    arr = _capi.make_cameras([rtw.t_default_cam(elem_type=T)] * n, T)
    if edit is not None:
        arr[edit[0]] = edit[1]
    return arr


def test_symbols_declared_exported_and_listed(lib, rtw):
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert len(SYMBOLS) == 10
    for name in SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
        assert not any(s in name for s in PINNED), name
    assert sorted(n for n in declared if "lens" in n) == sorted(SYMBOLS)
    assert sorted(n for n in _capi.SYMBOLS if "lens" in n) == sorted(SYMBOLS)
    assert sorted(set(re.findall(r"\b(rtw_\w*lens\w*)\b", exported))) == sorted(SYMBOLS)
    assert lib.rtw_abi_version() == 4                    # additive: the ABI version stays
    for name in PY_NAMES:
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name
    block = header[header.index("Batched lens stages: N views, or ONE frame under N lens settings"):header.index("rtw_lens_table_bytes(int32_t")]
    for word in ("Left out on purpose", "views of different sizes", "a batched motion", "device lists", "the Julia shim", "bit for bit", "n_frames is n_views",
                 "inputs counted once when n_frames == 1", "2^39", "detected by symbol lookup"):
        assert word in block, word


def test_work_and_table_bytes(lib):
    """the batch's workspace is n_views single ones; bad sizes, element sizes, radii and counts refused with the single stage's codes"""
    fn, one = lib.rtw_lens_batch_work_bytes, lib.rtw_wide_aperture_work_bytes
    for eb in (4, 8):
        for W, H in [(1, 1), (17, 33), (130, 5)]:
            for mr in (8, 16, 32):
                for nv in (1, 2, 3, 65537):
                    assert fn(W, H, eb, mr, nv) == nv * one(W, H, eb, mr) > 0, (W, H, eb, mr, nv)
        for size, code in BAD_SIZES:
            assert fn(*size, eb, 16, 2) == code, size
        for mr in (0, -1, 33):
            assert fn(10, 6, eb, mr, 2) == -2 and b"max_radius" in lib.rtw_last_error()
        for nv in (0, -1):
            assert fn(10, 6, eb, 16, nv) == -2 and b"n_views" in lib.rtw_last_error()
        assert fn(1 << 15, 1 << 15, eb, 16, 1 << 9) == -5 and b"too large" in lib.rtw_last_error()
        assert lib.rtw_lens_table_bytes(3, eb) == 32 * 3 * eb and lib.rtw_lens_table_bytes(0, eb) == -2 and b"n_views" in lib.rtw_last_error()
    assert fn(10, 6, 2, 16, 2) == -2 and lib.rtw_lens_table_bytes(3, 2) == -2 and b"elem_bytes" in lib.rtw_last_error()


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_lens_table_equals_its_restatement(lib, rtw, T):
    """rtw_lens_table_* on hand-made cameras, with and without per-view arrays and with a focus override: elements 0..28 are the
    reprojection table's entry of each camera as its own previous one (paths_ref.table), 29 and 30 defocus_ref.host_constants' F and K,
    31 is 0 -- on the bits"""
    from rtw_amd import _capi
    fn = getattr(lib, "rtw_lens_table_" + ("f64" if T is np.float64 else "f32"))
    W, H = 33, 17
    cams = [FO.handmade_camera(H, W, T), FO.handmade_camera(H, W, T, focus=5.0, origin=(-1.0, 0.5, 2.0)), FO.handmade_camera(H, W, T, focus=2.5, origin=(0.1, 0.2, 0.3)),
            rtw.t_default_cam(elem_type=T)]
    n = len(cams)
    arr = _capi.make_cameras(cams, T)
    for lens_radii, focus_dists in ((None, None), ([0.0, 0.125, 1 / 3, 2.5], None), (None, [0.0, 6.0, 0.7, 0.0]), ([0.3, 0.0, 1e-3, 0.75], [3.25, 0.0, 1e3, 0.0])):
        for b_lens, b_focus in ((0.05, 0.0), (0.4, 6.0)):
            got = np.full((n, 32), -7.0, T)
            assert fn(C.byref(_b(lens_radius=b_lens, focus_dist=b_focus)), arr, n, W, H, _dbl(lens_radii), _dbl(focus_dists), got.ctypes.data_as(C.c_void_p)) == 0
            ref = LB.lens_table(cams, T, W, lens_radii or [b_lens] * n, focus_dists or [b_focus] * n)
            assert FO.same_bits(got, ref), (lens_radii, focus_dists, b_lens, b_focus)
            assert not got[:, 31].any() and (got[:, 29] > 0).all()
    assert rtw.lens_table([c if isinstance(c, rtw.Camera) else LB.as_camera(c, T) for c in cams], W, H, lens_radii=[0.3, 0.0, 1e-3, 0.75], focus_dists=[3.25, 0.0, 1e3, 0.0]).tobytes() == ref.tobytes()
    assert lib.rtw_lens_table_bytes(n, np.dtype(T).itemsize) == ref.nbytes


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_lens_table_refuses(lib, rtw, T):
    fn = getattr(lib, "rtw_lens_table_" + ("f64" if T is np.float64 else "f32"))
    W, H, n = 10, 6, 3
    tab = np.zeros((n, 32), T)
    err = lib.rtw_last_error
    ref = lambda x: None if x is None else C.byref(x)

    def call(b="default", cams="default", nv=n, size=(W, H), lr=None, fd=None, t=tab.ctypes.data):
        return fn(ref(_b() if b == "default" else b), _cams(rtw, T, n) if cams == "default" else cams, nv, *size, _dbl(lr), _dbl(fd), C.c_void_p(t) if t else None)

    assert call() == 0
    assert call(b=None) == -1 and b"null" in err() and call(cams=None) == -1 and call(t=0) == -1
    assert call(nv=0) == -2 and b"n_views" in err() and call(nv=-3) == -2
    for bad in WAA.BAD_B:
        assert call(_b(**bad)) == -2, bad
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    for name, bad in _bad_cameras(rtw, T):
        assert call(cams=_cams(rtw, T, n, (1, bad))) == -2 and b"view 1" in err(), name
    for x in BAD_LENS + [-1.0]:                                     # (-1 is "the camera's own" in the one-call form alone)
        assert call(lr=[0.1, 0.2, x]) == -2 and b"view 2" in err() and b"lens_radius" in err(), x
    for x in BAD_FOCUS:
        assert call(fd=[x, 1.0, 2.0]) == -2 and b"view 0" in err() and b"focus_dist" in err(), x
    assert call(_b(lens_radius=float("nan")), lr=[0.1, 0.2, 0.3]) == 0                 # the arrays replace b's own values
    assert call(fd=[3.0, 3.0, 3.0], cams=_cams(rtw, T, n, (2, dict(_bad_cameras(rtw, T))["focus0"]))) == 0      # an override replaces the camera's own focus
    assert call(_b(max_radius=33), t=0) == -1                      # precedence: a null beats a bad parameter


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_device_form_is_refused_without_a_device(lib, T):
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_lens_batch_device_" + sfx)
    W, H, n = 10, 6, 3
    frame, feat_b, n_work = W * H * 3 * eb, W * H * 8 * eb, lib.rtw_wide_aperture_work_bytes(W, H, eb, 32)
    tab, img, feat, work, out = 0x80000, 0x100000, 0x200000, 0x400000, 0x500000       # never dereferenced
    assert work + n * n_work < out and lib.rtw_lens_batch_work_bytes(W, H, eb, 32, n) == n * n_work
    err = lib.rtw_last_error
    vp = lambda x: C.c_void_p(x) if x else None
    ref = lambda x: None if x is None else C.byref(x)

    def call(b="default", nv=n, nf=n, size=(W, H), t=tab, i=img, f=feat, w=work, o=out):
        return fn(ref(_b() if b == "default" else b), nv, nf, vp(t), *size, vp(i), vp(f), vp(w), vp(o), None)

    assert call(b=None) == -1 and b"null" in err()
    assert call(t=0) == -1 and call(i=0) == -1 and call(f=0) == -1 and call(w=0) == -1 and call(o=0) == -1
    assert call(nv=0, nf=0) == -2 and b"n_views" in err() and call(nv=-1, nf=1) == -2
    assert call(nf=2) == -2 and b"n_frames" in err() and call(nf=0) == -2 and call(nf=n + 1) == -2
    for bad in BAD_B_DEVICE:
        assert call(_b(**bad)) == -2, bad
    assert call(_b(max_radius=33)) == -2 and b"1..32" in err()
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    assert call(size=(1 << 15, 1 << 15), nv=1 << 9, nf=1) == -5 and b"too large" in err()
    assert call(t=tab + 8) == -2 and b"aligned" in err() and call(f=feat + 8) == -2 and call(w=work + 8) == -2 and call(i=img + 2) == -2 and call(o=out + 1) == -2
    # aliasing over the FULL batch extents: the last view's output, workspace and inputs count
    assert call(o=img + (n - 1) * frame + frame - eb) == -2 and b"alias" in err()
    assert call(o=feat + n * feat_b - eb) == -2 and call(o=work + n * n_work - eb) == -2 and call(o=tab + n * 32 * eb - eb) == -2
    assert call(w=out - n * n_work + 16) == -2 and b"alias" in err() and call(w=img + n * frame - 16) == -2 and call(w=out + n * frame - 16) == -2
    assert call(o=img - n * frame + eb) == -2                     # the LAST view's output reaches the first input frame
    # inputs counted once when n_frames == 1: behind frame 0 an output is free, and it is not with n_frames == n_views
    assert call(o=img + frame) == -2 and b"alias" in err()
    assert call(_b(max_radius=33), o=0) == -1                     # precedence: a null beats a bad parameter
    if not _has_gpu():
        rc = call()                                               # everything in order: only the device is missing
        assert rc not in (0, -1, -2, -5)
        assert call(nf=1, o=img + frame) == rc and call(nf=1, w=feat + feat_b) == rc
        assert call(nf=1, o=img + frame - eb) == -2
        for good in (dict(max_radius=1), dict(max_radius=8), dict(max_radius=9), dict(gamma=0), dict(lens_radius=float("nan")), dict(focus_dist=-1.0)):
            assert call(_b(**good)) == rc, good                   # of b only max_radius, gamma, device, flags and reserved are read
        assert call(_b(max_radius=8), o=work + n * lib.rtw_defocus_work_bytes(W, H, eb)) == rc        # the workspace's size follows max_radius
        assert call(nv=1, nf=1) == rc


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_host_form_is_refused_without_a_device(lib, rtw, T):
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_lens_batch_" + sfx)
    W, H, n = 10, 6, 3
    px = W * H
    sizes = dict(i=n * px * 3, f=n * px * 8, o=n * px * 3)
    buf = np.zeros(sum(sizes.values()) + 8, T)
    at, k = {}, 0
    for name, sz in sizes.items():
        at[name] = buf.ctypes.data + k * eb
        k += sz
    err = lib.rtw_last_error
    vp = lambda x: C.c_void_p(x) if x else None
    ref = lambda x: None if x is None else C.byref(x)

    def call(b="default", cams="default", nv=n, nf=n, lr=None, fd=None, size=(W, H), **ptr):
        a = dict(at)
        a.update(ptr)
        return fn(ref(_b() if b == "default" else b), _cams(rtw, T, n) if cams == "default" else cams, nv, nf, _dbl(lr), _dbl(fd), *size, vp(a["i"]), vp(a["f"]), vp(a["o"]))

    assert call(b=None) == -1 and b"null" in err() and call(cams=None) == -1 and call(i=0) == -1 and call(f=0) == -1 and call(o=0) == -1
    assert call(nv=0, nf=0) == -2 and b"n_views" in err() and call(nf=2) == -2 and b"n_frames" in err()
    for bad in WAA.BAD_B:
        assert call(_b(**bad)) == -2, bad
    for name, bad in _bad_cameras(rtw, T):
        assert call(cams=_cams(rtw, T, n, (2, bad))) == -2 and b"view 2" in err(), name
    for x in BAD_LENS + [-1.0]:
        assert call(lr=[x, 0.1, 0.1]) == -2 and b"view 0" in err(), x
    for x in BAD_FOCUS:
        assert call(fd=[1.0, x, 1.0]) == -2 and b"view 1" in err(), x
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    assert call(o=at["i"] + (n - 1) * px * 3 * eb) == -2 and b"alias" in err() and call(o=at["f"] + 16) == -2
    assert call(nf=1, o=at["i"] + px * 3 * eb - eb, f=at["o"]) == -2 and b"alias" in err()
    if not _has_gpu():
        rc = call()
        assert rc not in (0, -1, -2, -5)
        assert call(nf=1, o=at["i"] + px * 3 * eb, f=at["o"]) == rc    # one input frame: the bytes behind it are free (the one frame of features moved out of the way)
        assert call(_b(max_radius=1, lens_radius=0.0)) == rc and call(lr=[0.0, 0.5, 1.0], fd=[0.0, 2.0, 9.0]) == rc


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_one_call_form_is_refused_without_a_device(lib, rtw, T):
    """rtw_render_lens_batch_*: nulls (the filter, the seeds and the two arrays are optional), the stage's own refusals per view -- a lens
    radius of -1 is the camera's own here and only here --, and everything the batched render, feature pass and filter refuse"""
    from rtw_amd import _capi
    from rtw_amd.denoise import make_denoise
    sfx = "f64" if T is np.float64 else "f32"
    fn = getattr(lib, "rtw_render_lens_batch_" + sfx)
    W, H, n = 10, 6, 3
    S, keep = _capi.make_scene(rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T), T)
    cams = _capi.make_cameras([rtw.t_cam1(elem_type=T)] * n, T)
    assert cams[0].lens_radius > 0
    out = np.zeros(n * W * H * 3, T)
    err = lib.rtw_last_error
    P = lambda **kw: _capi.make_params(kw.pop("w", W), kw.pop("h", H), kw.pop("spp", 2), **kw)
    ref = lambda x: None if x is None else C.byref(x)

    def call(p="default", d=None, b="default", s=S, c=cams, nv=n, lr=None, fd=None, o=out.ctypes.data):
        return fn(ref(s), c, nv, None, ref(P() if p == "default" else p), ref(d), ref(_b() if b == "default" else b), _dbl(lr), _dbl(fd), C.c_void_p(o) if o else None)

    assert call(p=None) == -1 and b"null" in err() and call(b=None) == -1 and call(s=None) == -1 and call(c=None) == -1 and call(o=0) == -1
    assert call(nv=0) == -2 and call(nv=-2) == -2
    for bad in WAA.BAD_B:
        if bad != dict(lens_radius=-1.0):
            assert call(b=_b(**bad)) == -2, bad
    bad_cams = _capi.make_cameras([rtw.t_cam1(elem_type=T)] * n, T)
    bad_cams[1].lens_radius = -0.25
    assert call(b=_b(lens_radius=-1.0), c=bad_cams) == -2 and b"view 1" in err()          # the camera's own, and that is negative
    assert call(lr=[0.1, -1.0, 0.1], c=bad_cams) == -2 and b"view 1" in err()
    for x in BAD_LENS:
        assert call(lr=[0.1, 0.1, x]) == -2 and b"view 2" in err(), x
    for x in BAD_FOCUS:
        assert call(fd=[x, 0.0, 0.0]) == -2 and b"view 0" in err(), x
    for name, bad in _bad_cameras(rtw, T):
        c2 = _capi.make_cameras([rtw.t_cam1(elem_type=T)] * n, T)
        c2[2] = bad
        assert call(c=c2) == -2, name
    for size, code in BAD_SIZES:
        assert call(P(w=size[0], h=size[1])) == code, size
    assert call(P(spp=0)) == -2 and call(P(flags=_capi.FLAG_COMPACT_TILES)) == -2 and call(d=make_denoise(levels=0)) == -2
    bad_scene, keep2 = _capi.make_scene(rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T), T)
    bad_scene.n = -1
    assert call(s=bad_scene) == -2 and b"sphere count" in err()
    if not _has_gpu():
        rc = call()
        assert rc not in (0, -1, -2, -4, -5)                  # everything in order: only the device is missing
        assert call(b=_b(lens_radius=-1.0)) == rc and call(d=make_denoise()) == rc and call(lr=[-1.0, 0.2, 0.0], fd=[0.0, 7.0, 0.0]) == rc and call(b=_b(max_radius=3)) == rc
    del keep, keep2


def test_the_python_layer_checks_its_arguments(rtw):
    T = np.float32
    cam = rtw.t_default_cam(elem_type=T)
    imgs, feats = np.zeros((2, 6, 10, 3), T), np.zeros((2, 6, 10, 8), T)
    with pytest.raises(ValueError):
        rtw.wide_aperture_batch(imgs[0], feats[0], [cam, cam], lens_radius=0.1)
    with pytest.raises(ValueError):
        rtw.wide_aperture_batch(imgs, feats, [cam], lens_radius=0.1)
    with pytest.raises(ValueError):
        rtw.wide_aperture_batch(imgs, feats, [cam, cam], lens_radii=[0.1])
    with pytest.raises(TypeError):
        rtw.wide_aperture_batch(imgs, feats.astype(np.float64), [cam, cam], lens_radius=0.1)
    with pytest.raises(TypeError):
        rtw.wide_aperture_batch(imgs, feats, [cam, rtw.t_default_cam(elem_type=np.float64)], lens_radius=0.1)
    with pytest.raises(ValueError):
        rtw.focus_bracket(imgs[0], feats[0], cam, lens_radius=0.1)
    with pytest.raises(ValueError):
        rtw.focus_bracket(imgs[0], feats[0], cam, focus_dists=[1.0, 2.0], lens_radii=[0.1])
    with pytest.raises(Exception) as e:
        rtw.focus_bracket(imgs[0], feats[0], cam, focus_dists=[1.0, -2.0], lens_radius=0.1)
    assert "view 1" in str(e.value) and "focus_dist" in str(e.value)
    with pytest.raises(ValueError):
        rtw.render_wide_aperture_batch(rtw.scene_2_spheres(elem_type=T), [cam, cam], 16, 1, lens_radii=[0.1])
    with pytest.raises(ValueError):
        rtw.render_wide_aperture_batch(rtw.scene_2_spheres(elem_type=T), [], 16, 1)
    assert rtw.wide_aperture_batch_work_bytes(96, 54, 5) == 5 * rtw.wide_aperture_work_bytes(96, 54)
    assert rtw.wide_aperture_batch_work_bytes(96, 54, 2, np.float64, 8) == 2 * rtw.defocus_work_bytes(96, 54, np.float64)


def test_c_example_compiles_and_links(tmp_path):
    """examples/render_focus_bracket_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_focus_bracket_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "render_focus_bracket_c.c"),
                        "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "2"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr
