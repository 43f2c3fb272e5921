"""Batched temporal steps, CPU only (include/rtw_hip.h rtw_reproject_*, rtw_render_paths_*): the nine symbols are declared, listed and
exported and form a closed set, the table's size and content are what the header says -- on the bits, against temporal_ref.host_constants and
the camera fields --, and every refusal of every entry point is decided before any HIP call (the dummy device pointers below are never
dereferenced)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import paths_ref as PR
import temporal_ref as TR
from conftest import ROOT

PATHS_SYMBOLS = ["rtw_reproject_table_bytes", "rtw_reproject_table_f32", "rtw_reproject_table_f64", "rtw_reproject_batch_device_f32", "rtw_reproject_batch_device_f64",
                 "rtw_reproject_noise_batch_device_f32", "rtw_reproject_noise_batch_device_f64", "rtw_render_paths_f32", "rtw_render_paths_f64"]
PY_NAMES = ("temporal_path_table", "temporal_step_batch_into", "temporal_noise_batch_into", "TemporalBatchAccumulator", "render_sequences")
TYPES = [np.float32, np.float64]


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


def _c(**kw):
    from rtw_amd import _capi
    v = dict(radius=1, flags=0, reserved=(0, 0), sigma=1.0, len_scale=0.5)
    v.update(kw)
    v["reserved"] = (C.c_int32 * 2)(*v["reserved"])
    return _capi.TemporalClamp(**v)


def _n(**kw):
    from rtw_amd import _capi
    v = dict(radius=2, normal_power_log2=1, device=-1, reserved=(0, 0, 0), sigma_depth=0.1, min_len=4.0)
    v.update(kw)
    v["reserved"] = (C.c_int32 * 3)(*v["reserved"])
    return _capi.TemporalNoise(**v)


BAD_T = [dict(normal_power_log2=8), dict(flags=2), dict(gamma=2), dict(device=-2), dict(reserved=(1, 0)), dict(sigma_depth=0.0), dict(min_weight=1.5),
         dict(history_max=float("nan"))]
BAD_C = [dict(radius=0), dict(radius=4), dict(flags=2), dict(reserved=(0, 1)), dict(sigma=-1.0), dict(sigma=float("inf")), dict(len_scale=1.5), dict(len_scale=float("nan"))]
BAD_N = [dict(radius=0), dict(radius=4), dict(normal_power_log2=8), dict(device=-2), dict(reserved=(0, 0, 1)), dict(sigma_depth=0.0), dict(min_len=0.5)]
BAD_SIZES = [((0, 3), -2), ((5, 0), -2), ((-5, 3), -2), ((2 ** 31 - 1, 2 ** 31 - 1), -5)]


def test_the_nine_symbols_are_declared_exported_listed_and_closed(lib, rtw):
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in PATHS_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert sorted(n for n in declared if "reproject" in n or "render_paths" in n) == sorted(PATHS_SYMBOLS)
    assert lib.rtw_abi_version() == 4                    # additive: the ABI version stays
    for name in PY_NAMES:
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name
    # the three temporal blocks no longer list several paths per launch as left out; the new block has its own list
    assert "N sequences per launch" not in header and "N independent sequences in one launch" not in header
    block = header[header.index("Batched temporal steps"):header.index("rtw_reproject_table_bytes(")]
    assert "Left out on purpose" in block and "detected by symbol lookup" in block


def test_table_bytes(lib):
    tb = lib.rtw_reproject_table_bytes
    for n in (1, 3, 65535, 65536, 2 ** 31 - 1):
        assert tb(n, 4) == n * 128 and tb(n, 8) == n * 256
    for args in ((0, 4), (-1, 4), (3, 2), (3, 0), (3, 16)):
        assert tb(*args) == -2, args
    assert tb(3, 3) == -2 and b"elem_bytes" in lib.rtw_last_error()


@pytest.mark.parametrize("T", TYPES)
def test_the_table_equals_the_host_constants_on_the_bits(lib, rtw, T):
    """the three test paths: current cameras at step 1, previous ones at step 0; with and without cams_prev; through the C ABI and through Python"""
    from rtw_amd import _capi
    fn = getattr(lib, "rtw_reproject_table_" + ("f64" if T is np.float64 else "f32"))
    for W, H in ((37, 23), (5, 3)):
        cams = [PR.path_cameras(T, s, W, H)[0] for s in range(PR.N_PATHS)]
        cur, prev = [c[1] for c in cams], [c[0] for c in cams]
        for cp in (prev, None):
            ref = PR.table(cur, cp, T)
            got = np.full((PR.N_PATHS + 1, 32), -7.0, T)
            assert fn(_capi.make_cameras(cur, T), _capi.make_cameras(cp, T) if cp else None, PR.N_PATHS, got.ctypes.data_as(C.c_void_p)) == 0
            assert TR.same_bits(got[:PR.N_PATHS], ref), (W, H, cp is None)
            assert (got[PR.N_PATHS] == -7.0).all()                      # nothing behind the last entry is written
            assert not got[:PR.N_PATHS, 29:].any() and (cp is not None or not got[:PR.N_PATHS, 12:].any())
            py = rtw.temporal_path_table(cur, cp)
            assert py.shape == (PR.N_PATHS, 32) and py.dtype == T and TR.same_bits(py, ref)
        # one entry alone is the single call's constants: Kw .. iv as temporal_ref.host_constants states them
        K = TR.host_constants(prev[1], T, 0.1, 0.25, 16.0)
        one = rtw.temporal_path_table([cur[1]], [prev[1]])
        assert TR.same_bits(one[0, 24:29], np.array([K[k] for k in ("Kw", "Qh", "Qv", "ih", "iv")], T))
    cam = _capi.make_cameras([rtw.t_default_cam(elem_type=T)], T)
    buf = np.zeros(32, T)
    assert fn(None, None, 1, buf.ctypes.data_as(C.c_void_p)) == -1 and fn(cam, None, 1, None) == -1 and b"null" in lib.rtw_last_error()
    assert fn(cam, None, 0, buf.ctypes.data_as(C.c_void_p)) == -2 and fn(cam, None, -3, buf.ctypes.data_as(C.c_void_p)) == -2 and b"n_paths" in lib.rtw_last_error()
    with pytest.raises(ValueError):
        rtw.temporal_path_table([rtw.t_default_cam(elem_type=T)] * 2, [rtw.t_default_cam(elem_type=T)])
    with pytest.raises(TypeError):
        rtw.temporal_path_table([rtw.t_default_cam(elem_type=np.float32), rtw.t_default_cam(elem_type=np.float64)])


@pytest.mark.parametrize("T", TYPES)
def test_the_batched_step_is_refused_without_a_device(lib, T):
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_reproject_batch_device_" + sfx)
    W, H, S = 9, 7, 3                                     # W*H odd: the strides carry padding
    n_img, n_feat = S * W * H * 3 * eb, S * W * H * 8 * eb
    n_st, n_mo, n_tab = S * lib.rtw_temporal_state_bytes(W, H, eb), S * lib.rtw_history_moment_bytes(W, H, eb), S * 32 * eb
    tab, img, feat, sp, mp, sn, mn, out = (0x100000 * k for k in range(1, 9))       # never dereferenced
    err = lib.rtw_last_error

    def call(t=None, c=None, s=S, size=(W, H), tb=tab, i=img, f=feat, p=sp, q=mp, n=sn, m=mn, o=out, no_t=False, clamp=True):
        t = _t() if t is None else t
        c = _c() if c is None else c
        vp = lambda x: C.c_void_p(x) if x else None
        return fn(None if no_t else C.byref(t), C.byref(c) if clamp else None, s, vp(tb), *size, vp(i), vp(f), vp(p), vp(q), vp(n), vp(m), vp(o), None)

    assert call(no_t=True) == -1 and b"null" in err()
    assert call(tb=0) == -1 and call(i=0) == -1 and call(f=0) == -1 and call(n=0) == -1 and call(o=0) == -1
    assert call(m=0) == -1                               # a previous moment plane without a next one
    assert call(s=0) == -2 and call(s=-1) == -2 and b"n_paths" in err()
    for bad in BAD_T:
        assert call(_t(**bad)) == -2, bad
    for bad in BAD_C:
        assert call(c=_c(**bad)) == -2, bad
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    # the batched filter's frame rule on (width, height, number of paths)
    assert call(size=(1 << 15, 1 << 15), s=1 << 9) == -5 and b"too large" in err()
    # exactly one of d_states_prev / d_moments_prev with moments on
    assert call(q=0) == -2 and b"both" in err()
    assert call(p=0) == -2 and b"both" in err()
    # alignment: 16 bytes for the table, features, states and moment planes; T for images and out
    for k in ("tb", "f", "p", "q", "n", "m"):
        assert call(**{k: dict(tb=tab, f=feat, p=sp, q=mp, n=sn, m=mn)[k] + 8}) == -2 and b"aligned" in err(), k
    assert call(i=img + 2) == -2 and call(o=out + 2) == -2 and b"aligned" in err()
    # aliasing over the extents of ALL paths: an output that starts inside the last path of another buffer, or ends inside its first
    assert call(o=sn) == -2 and b"alias" in err()
    assert call(o=sn + n_st - eb) == -2 and call(o=sn - n_img + eb) == -2 and call(o=mn + n_mo - eb) == -2
    for base, size in ((img, n_img), (feat, n_feat), (sp, n_st), (mp, n_mo), (tab, n_tab)):
        assert call(o=base + size - eb) == -2 and call(o=base - n_img + eb) == -2 and b"alias" in err(), hex(base)
        assert call(n=base + size - 16) == -2 and call(n=base - n_st + 16) == -2, hex(base)
        assert call(m=base + size - 16) == -2 and call(m=base - n_mo + 16) == -2, hex(base)
    assert call(m=sn + n_st - 16) == -2
    # the extents are the batch's: one path's extent behind the first path of a buffer still aliases
    one_st = n_st // S
    assert call(n=sp + one_st) == -2 and call(o=img + n_img // S) == -2
    assert call(_t(gamma=9), o=0) == -1                  # a null beats a bad parameter
    assert call(_t(gamma=9), s=0) == -2
    if not _has_gpu():
        rc = call()                                      # everything in order: only the device is missing
        assert rc not in (0, -1, -2, -5)
        assert call(clamp=False) == rc and call(q=0, m=0) == rc and call(clamp=False, q=0, m=0) == rc       # plain steps; no moments
        assert call(p=0, q=0) == rc and call(p=0, q=0, o=sp) == rc                                         # first frames: no previous state to alias
        assert call(s=1) == rc and call(s=20) == rc


@pytest.mark.parametrize("T", TYPES)
def test_the_batched_noise_map_is_refused_without_a_device(lib, T):
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_reproject_noise_batch_device_" + sfx)
    W, H, S = 9, 7, 3
    n_st, n_mo, n_rho = S * lib.rtw_temporal_state_bytes(W, H, eb), S * lib.rtw_history_moment_bytes(W, H, eb), S * W * H * eb
    st, mo, rho = 0x100000, 0x200000, 0x300000
    err = lib.rtw_last_error

    def call(n=None, size=(W, H), s=S, a=st, b=mo, r=rho, no_n=False):
        n = _n() if n is None else n
        vp = lambda x: C.c_void_p(x) if x else None
        return fn(None if no_n else C.byref(n), *size, s, vp(a), vp(b), vp(r), None)

    assert call(no_n=True) == -1 and call(a=0) == -1 and call(b=0) == -1 and call(r=0) == -1 and b"null" in err()
    assert call(s=0) == -2 and call(s=-4) == -2 and b"n_paths" in err()
    for bad in BAD_N:
        assert call(_n(**bad)) == -2, bad
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    assert call(size=(1 << 15, 1 << 15), s=1 << 9) == -5 and b"too large" in err()
    assert call(a=st + 8) == -2 and call(b=mo + 8) == -2 and call(r=rho + 2) == -2 and b"aligned" in err()
    assert call(r=st + n_st - eb) == -2 and call(r=st - n_rho + eb) == -2 and call(r=mo + n_mo - eb) == -2 and call(r=mo - n_rho + eb) == -2 and b"alias" in err()
    assert call(_n(radius=9), r=0) == -1
    if not _has_gpu():
        assert call() not in (0, -1, -2, -5) and call(s=1) not in (0, -1, -2, -5)


@pytest.mark.parametrize("T", TYPES)
def test_render_paths_is_refused_without_a_device(lib, rtw, T):
    """nulls, the counts and their product, the forms' rules, the step's, the clamp's and the noise map's own checks, and everything the batched
    render, feature and filter calls refuse for n_steps*n_paths views"""
    from rtw_amd import _capi
    sfx = "f64" if T is np.float64 else "f32"
    fn = getattr(lib, "rtw_render_paths_" + sfx)
    S, keep = _capi.make_scene(rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T), T)
    NP, NS = 2, 3
    cams = _capi.make_cameras([rtw.t_default_cam(elem_type=T)] * (NP * NS), T)
    out = np.zeros(NP * NS * 96 * 54 * 3, T)
    D = _capi.Denoise(3, 1, 1, 1, -1, 0, 0.5, 0.1)
    err = lib.rtw_last_error
    ref = lambda x: C.byref(x) if x is not None else None

    def call(P, t=None, c=None, n=None, d=None, scene=S, cm=cams, o=out, no_t=False, np_=NP, ns=NS):
        t = _t() if t is None else t
        return fn(ref(scene), cm, np_, ns, None, ref(P), None if no_t else C.byref(t), ref(c), ref(n), ref(d), o.ctypes.data_as(C.c_void_p) if o is not None else None)

    P = _capi.make_params(96, 54, 4)
    assert call(None) == -1 and call(P, scene=None) == -1 and call(P, cm=None) == -1 and call(P, o=None) == -1 and call(P, no_t=True) == -1 and b"null" in err()
    assert call(P, np_=0) == -2 and call(P, ns=0) == -2 and call(P, np_=-1) == -2 and b"n_paths" in err()
    assert call(P, np_=1 << 16, ns=1 << 15) == -2 and b"32 bits" in err()
    assert call(P, n=_n()) == -2 and b"d is required" in err()                      # n without d
    assert call(P, n=_n(), d=_capi.Denoise(3, 1, 0, 1, -1, 0, 0.5, 0.1)) == -2 and b"DEMODULATE" in err()
    for forms in (dict(), dict(c=_c()), dict(d=D), dict(c=_c(), d=D), dict(n=_n(), d=D), dict(c=_c(), n=_n(), d=D)):
        for bad in BAD_T:
            assert call(P, _t(**bad), **forms) == -2, (bad, forms)
        assert call(None, _t(gamma=9), **forms) == -1                               # a null beats a bad parameter
    for bad in BAD_C:
        assert call(P, c=_c(**bad)) == -2, bad
    for bad in BAD_N:
        assert call(P, n=_n(**bad), d=D) == -2, bad
    for bad in (dict(levels=0), dict(levels=9), dict(flags=2), dict(gamma=2), dict(sigma_color=0.0)):
        v = dict(levels=3, normal_power_log2=1, flags=1, gamma=1, device=-1, reserved=0, sigma_color=0.5, sigma_depth=0.1)
        v.update(bad)
        assert call(P, d=_capi.Denoise(**v)) == -2, bad
    # what a batched render / feature render refuses
    assert call(_capi.make_params(96, 54, 4, shard_index=0, shard_count=2)) == -2 and b"shard_count" in err()
    assert call(_capi.make_params(96, 54, 4, flags=_capi.FLAG_COMPACT_TILES)) == -2 and b"COMPACT_TILES" in err()
    assert call(_capi.make_params(96, 54, 4, devices=[0, 1])) == -2 and b"n_devices" in err()
    assert call(_capi.make_params(0, 54, 4)) == -2 and call(_capi.make_params(96, 54, 0)) == -2
    assert call(_capi.make_params(2 ** 31 - 1, 2 ** 31 - 1, 4)) == -5
    if not _has_gpu():
        assert call(P) not in (0, -1, -2, -5) and b"no HIP device" in err()
        for forms in (dict(c=_c()), dict(d=D), dict(c=_c(), n=_n(), d=D)):
            assert call(P, **forms) not in (0, -1, -2, -5), forms
        assert call(P, np_=1, ns=1) not in (0, -1, -2, -5)
    del keep


def test_python_validation(rtw):
    T = np.float32
    cam, cam64 = rtw.t_default_cam(elem_type=T), rtw.t_default_cam(elem_type=np.float64)
    scene = rtw.scene_2_spheres(elem_type=T)
    with pytest.raises(ValueError):
        rtw.render_sequences(scene, [], 96, 4)
    with pytest.raises(ValueError):
        rtw.render_sequences(scene, [[cam, cam], [cam]], 96, 4)
    with pytest.raises(ValueError):
        rtw.render_sequences(scene, [[cam, cam], [cam, cam]], 96, 4, seeds=[[1, 2]])
    with pytest.raises(TypeError):
        rtw.render_sequences(scene, [[cam, cam], [cam, cam64]], 96, 4)
    with pytest.raises(ValueError, match="keywords"):
        rtw.render_sequences(scene, [[cam, cam]], 96, 4, clamp=dict(gamma=1))
    with pytest.raises(ValueError):
        rtw.temporal_step_batch_into(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 2, 5, 3, clamp=dict(bogus=1))
    assert "step-major" in rtw.render_sequences.__doc__ and "ONE launch" in rtw.temporal_step_batch_into.__doc__


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_paths_fail_loudly_without_gpu(rtw):
    from rtw_amd._capi import RtwError
    T = np.float32
    cam = rtw.t_default_cam(elem_type=T)
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.render_sequences(rtw.scene_2_spheres(elem_type=T), [[cam, cam], [cam, cam]], 96, 4)
    with pytest.raises(RtwError, match="device"):
        rtw.temporal_step_batch_into(0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 2, 5, 3)


def test_c_stereo_example_compiles_and_links(tmp_path):
    """examples/render_stereo_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_stereo_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "render_stereo_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "2", "3"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode != 0 and "no HIP device" in (r.stdout + r.stderr)
