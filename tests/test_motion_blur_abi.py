"""The motion-blur stage, CPU only (include/rtw_hip.h rtw_velocity_blur_*, rtw_render_blurred_*): the symbols are declared, listed and
exported, the struct and the workspace have the sizes the header says, and every refusal of every new entry point is decided before any
HIP call (the dummy device pointers below are never dereferenced)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import motion_blur_ref as BR
from conftest import ROOT
from test_temporal_clamp_abi import BAD_C, _c
from test_temporal_noise_abi import BAD_SIZES, BAD_T, _has_gpu, _t

BLUR_SYMBOLS = ["rtw_velocity_blur_work_bytes", "rtw_velocity_blur_device_f32", "rtw_velocity_blur_device_f64", "rtw_velocity_blur_f32", "rtw_velocity_blur_f64",
                "rtw_render_blurred_f32", "rtw_render_blurred_f64"]
PY_NAMES = ["make_motion_blur", "motion_blur_work_bytes", "motion_blur", "motion_blur_into"]
BAD_B = [dict(taps=1), dict(taps=2), dict(taps=4), dict(taps=14), dict(taps=33), dict(taps=-3), dict(flags=1), dict(flags=-1), dict(gamma=2), dict(gamma=-1), dict(device=-2),
         dict(reserved=(1, 0)), dict(reserved=(0, -1)), dict(shutter=0.0), dict(shutter=-0.5), dict(shutter=1.5), dict(shutter=float("nan")), dict(shutter=float("inf")),
         dict(depth_extent=0.0), dict(depth_extent=-1.0), dict(depth_extent=float("inf")), dict(depth_extent=float("nan"))]
GOOD_B = [dict(taps=3), dict(taps=31), dict(shutter=1.0), dict(shutter=1e-6), dict(depth_extent=1e-9), dict(depth_extent=1e9), dict(gamma=0), dict(device=0)]


@pytest.fixture(scope="module")
def lib(rtw):
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def _b(**kw):
    from rtw_amd import _capi
    v = dict(taps=15, flags=0, gamma=1, device=-1, reserved=(0, 0), shutter=1.0, depth_extent=0.5)
    v.update(kw)
    v["reserved"] = (C.c_int32 * 2)(*v["reserved"])
    return _capi.VelocityBlur(**v)


def test_symbols_declared_exported_and_listed(lib, rtw):
    import inspect
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in BLUR_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert sorted(n for n in declared if "blur" in n) == sorted(BLUR_SYMBOLS)
    assert lib.rtw_abi_version() == 4                    # additive: the ABI version stays
    for name in PY_NAMES:
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name
    assert "blur" in inspect.signature(rtw.render_animation).parameters
    assert C.sizeof(_capi.VelocityBlur) == 40 and re.search(r"\}\s*rtw_velocity_blur_t;\s*/\* 40 bytes \*/", header)
    assert re.search(r"#define\s+RTW_VELOCITY_BLUR_TILE\s+16\b", header)
    block = header[header.index("Motion blur: a velocity-guided gather"):header.index("rtw_velocity_blur_work_bytes(int32_t")]
    for word in ("Left out on purpose", "batched views", "device lists", "the Julia shim", "jittered taps", "lens-aware velocities", "never", "lowest slot", "ties to even"):
        assert word in block, word
    # the motion block no longer lists the blur as left out: what stays out is a time per ray
    motion = header[header.index("Temporal reuse over moving spheres"):header.index("rtw_motion_table_f32(")]
    assert "motion blur inside a frame" not in motion and "a time per ray" in motion


def test_work_bytes(lib):
    """the blur plane and two tile planes of 4-element slots: a multiple of 16, monotone in the size, the witness's count; bad sizes refused"""
    fn = lib.rtw_velocity_blur_work_bytes
    for eb in (4, 8):
        prev = 0
        for W, H in [(1, 1), (5, 3), (16, 16), (17, 16), (16, 17), (37, 23), (70, 40), (128, 72), (1920, 1080)]:
            n = fn(W, H, eb)
            assert n == BR.work_elems(H, W) * eb and n % 16 == 0 and n >= prev > -1, (W, H, eb)
            prev = n
        for W in range(1, 40):
            assert fn(W, 7, eb) <= fn(W + 1, 7, eb) and fn(7, W, eb) <= fn(7, W + 1, eb)
        for size, code in BAD_SIZES:
            assert fn(*size, eb) == code, size
    assert fn(10, 6, 2) == -2 and fn(10, 6, 16) == -2


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_device_form_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_velocity_blur_device_" + sfx)
    W, H = 10, 6
    n_img, n_feat, n_mv, n_work = W * H * 3 * eb, W * H * 8 * eb, W * H * 4 * eb, lib.rtw_velocity_blur_work_bytes(W, H, eb)
    img, feat, mv, work, out = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000       # never dereferenced
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    err = lib.rtw_last_error
    vp = lambda x: C.c_void_p(x) if x else None
    ref = lambda x: None if x is None else C.byref(x)

    def call(b="default", size=(W, H), c=cam, cp=cam, i=img, f=feat, v=mv, w=work, o=out):
        return fn(ref(_b() if b == "default" else b), ref(c), ref(cp), *size, vp(i), vp(f), vp(v), vp(w), vp(o), None)

    assert call(b=None) == -1 and b"null" in err()
    assert call(c=None) == -1 and call(cp=None) == -1 and call(i=0) == -1 and call(f=0) == -1 and call(v=0) == -1 and call(w=0) == -1 and call(o=0) == -1
    for bad in BAD_B:
        assert call(_b(**bad)) == -2, bad
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    assert call(f=feat + 8) == -2 and b"aligned" in err() and call(v=mv + 8) == -2 and call(w=work + 8) == -2 and call(i=img + 2) == -2 and call(o=out + 1) == -2
    assert call(o=img) == -2 and b"alias" in err() and call(o=feat + n_feat - eb) == -2 and call(o=mv + n_mv - eb) == -2 and call(o=work + n_work - eb) == -2
    assert call(w=img) == -2 and b"alias" in err() and call(w=feat + 16) == -2 and call(w=mv + n_mv - 16) == -2 and call(w=out - n_work + 16) == -2
    assert call(_b(taps=4), o=0) == -1                  # precedence: a null beats a bad parameter
    if not _has_gpu():
        rc = call()                                     # everything in order: only the device is missing
        assert rc not in (0, -1, -2, -5)
        for good in GOOD_B:
            if good != dict(device=0):
                assert call(_b(**good)) == rc, good


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_host_form_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_velocity_blur_" + sfx)
    W, H = 10, 6
    n = W * H
    sizes = dict(i=n * 3, f=n * 8, v=n * 4, o=n * 3)
    buf = np.zeros(sum(sizes.values()) + 8, T)
    at, k = {}, 0
    for name, sz in sizes.items():
        at[name] = buf.ctypes.data + k * eb
        k += sz
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    err = lib.rtw_last_error
    vp = lambda x: C.c_void_p(x) if x else None
    ref = lambda x: None if x is None else C.byref(x)

    def call(b="default", size=(W, H), c=cam, cp=cam, **ptr):
        a = dict(at)
        a.update(ptr)
        return fn(ref(_b() if b == "default" else b), ref(c), ref(cp), *size, vp(a["i"]), vp(a["f"]), vp(a["v"]), vp(a["o"]))

    assert call(b=None) == -1 and call(c=None) == -1 and call(cp=None) == -1 and call(i=0) == -1 and call(f=0) == -1 and call(v=0) == -1 and call(o=0) == -1
    for bad in BAD_B:
        assert call(_b(**bad)) == -2, bad
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    assert call(o=at["i"]) == -2 and b"alias" in err() and call(o=at["f"] + 16) == -2 and call(o=at["v"]) == -2
    if not _has_gpu():
        rc = call()
        assert rc not in (0, -1, -2, -5)
        assert call(_b(taps=3, shutter=0.25)) == rc


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_blurred_animation_is_refused_without_a_device(lib, rtw, T):
    """rtw_render_blurred_*: nulls (the blur's parameters are not optional), the blur's own refusals, and everything rtw_render_animation_*
    refuses -- all before any HIP call"""
    from rtw_amd import _capi
    from rtw_amd.denoise import make_denoise
    sfx = "f64" if T is np.float64 else "f32"
    fn = getattr(lib, "rtw_render_blurred_" + sfx)
    W, H, N = 10, 6, 3
    flat = rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T)
    made = [_capi.make_scene(flat, T) for _ in range(N)]
    scenes = (type(made[0][0]) * N)(*[m[0] for m in made])
    cams = _capi.make_cameras([rtw.t_default_cam(elem_type=T)] * N, T)
    seeds = _capi.make_seeds(3, N)
    out = np.zeros(N * W * H * 3, T)
    err = lib.rtw_last_error
    P = lambda **kw: _capi.make_params(kw.pop("w", W), kw.pop("h", H), kw.pop("spp", 2), **kw)
    ref = lambda x: None if x is None else C.byref(x)

    def call(p="default", t="default", k=None, d=None, b="default", s=scenes, c=cams, n=N, sd=seeds, o=out.ctypes.data):
        return fn(s, c, n, sd, ref(P() if p == "default" else p), ref(_t() if t == "default" else t), ref(k), ref(d), ref(_b() if b == "default" else b),
                  C.c_void_p(o) if o else None)

    assert call(p=None) == -1 and b"null" in err() and call(t=None) == -1 and call(b=None) == -1 and call(s=None) == -1 and call(c=None) == -1 and call(o=0) == -1
    for n in (0, -1, -7):
        assert call(n=n) == -2 and b"n_frames" in err(), n
    for bad in BAD_B:
        assert call(b=_b(**bad)) == -2, bad
    for bad in BAD_T:
        assert call(t=_t(**bad)) == -2, bad
    for bad in BAD_C:
        assert call(k=_c(**bad)) == -2, bad
    for size, code in BAD_SIZES:
        assert call(P(w=size[0], h=size[1])) == code, size
    assert call(P(spp=0)) == -2 and call(P(device=-2)) == -2 and call(P(flags=_capi.FLAG_COMPACT_TILES)) == -2 and call(d=make_denoise(levels=0)) == -2
    bad = (type(made[0][0]) * N)(*[m[0] for m in made])
    bad[N - 1].n = -1
    assert call(s=bad) == -2 and b"sphere count" in err()
    if not _has_gpu():
        rc = call()
        assert rc not in (0, -1, -2, -4, -5)                  # everything in order: only the device is missing
        assert call(sd=None) == rc and call(k=_c()) == rc and call(d=make_denoise()) == rc and call(n=1) == rc
    del made


def test_the_python_layer_checks_its_arguments(rtw):
    T = np.float32
    cam = rtw.t_default_cam(elem_type=T)
    img, feat, mv = np.zeros((6, 10, 3), T), np.zeros((6, 10, 8), T), np.zeros((6, 10, 4), T)
    with pytest.raises(TypeError):
        rtw.motion_blur(img, feat, mv.astype(np.float64), cam, cam)
    with pytest.raises(ValueError):
        rtw.motion_blur(img, feat, mv[:, :5], cam, cam)
    with pytest.raises(TypeError):
        rtw.motion_blur(img, feat, mv, cam, None)
    with pytest.raises(Exception) as e:
        rtw.motion_blur(img, feat, mv, cam, cam, taps=4)
    assert "taps" in str(e.value)
    with pytest.raises(ValueError):
        rtw.render_animation([rtw.scene_2_spheres(elem_type=T)], [cam], 16, 1, blur=dict(radius=3))
    assert rtw.motion_blur_work_bytes(70, 40) == BR.work_elems(40, 70) * 4 and rtw.motion_blur_work_bytes(70, 40, np.float64) == BR.work_elems(40, 70) * 8


def test_c_example_compiles_and_links(tmp_path):
    """examples/render_animation_blurred_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_animation_blurred_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "render_animation_blurred_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "2", "3"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr
