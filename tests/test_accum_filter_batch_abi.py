"""Batched passes over accumulators, CPU only (include/rtw_hip.h rtw_accum_resolve_batch_*, rtw_accum_features_batch_*, rtw_accum_noise_batch_*,
rtw_guided_filter_batch_device_*, rtw_accum_filtered_batch_*): the symbols are declared, listed and exported, and every refusal that does
not need a live handle is decided before any HIP call (the dummy handles and device pointers below are never dereferenced; a handle given
twice is found by comparing the pointers).  The refusals that look INTO an accumulator -- its kind, its binding, its intervals, its size --
need real ones: tests/test_gpu_accum_filter_batch.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_accum_denoise_abi import BAD_DENOISE, _bad_params, _d, _has_gpu

NEW_SYMBOLS = ["rtw_accum_resolve_batch_f32", "rtw_accum_resolve_batch_f64", "rtw_accum_features_batch_f32", "rtw_accum_features_batch_f64",
               "rtw_accum_noise_batch_f32", "rtw_accum_noise_batch_f64", "rtw_guided_filter_batch_device_f32", "rtw_guided_filter_batch_device_f64",
               "rtw_accum_filtered_batch_f32", "rtw_accum_filtered_batch_f64"]
PRECISIONS = [np.float32, np.float64]


@pytest.fixture(scope="module")
def lib(rtw):
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def _handles(*values):
    """a ctypes array of accumulator handles that are never dereferenced (0: a null entry)"""
    return (C.c_void_p * len(values))(*values)


DUMMIES = (0x1000, 0x2000, 0x3000)


def test_symbols_declared_exported_and_listed(lib, rtw):
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert lib.rtw_abi_version() == 4                    # additive: the ABI version stays
    for name in ("render_adaptive_denoised_batch", "denoise_guided_batch_into"):
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name
    for cls, names in ((rtw.ProgressiveBatchRenderer, ("features_all", "features_all_into", "denoised_all", "images_into", "denoised")),
                       (rtw.AdaptiveBatchRenderer, ("noise_all", "noise_all_into", "denoised_all", "features_all", "denoised"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)


@pytest.mark.parametrize("T", PRECISIONS)
def test_the_batched_resolve_and_noise_map_are_refused_without_a_device(lib, T):
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    resolve, noise = getattr(lib, "rtw_accum_resolve_batch_" + sfx), getattr(lib, "rtw_accum_noise_batch_" + sfx)
    err = lib.rtw_last_error
    out = 0x200000
    calls = {"resolve": lambda h, n, o=out: resolve(h, n, 1, C.c_void_p(o), None), "noise": lambda h, n, o=out: noise(h, n, C.c_void_p(o), None)}
    for name, call in calls.items():
        h3 = _handles(*DUMMIES)
        assert call(None, 3) == -1 and b"null" in err(), name
        assert call(h3, 3, o=0) == -1, name
        assert call(h3, 0) == -2 and b"n_views" in err(), name
        assert call(h3, -4) == -2, name
        assert call(_handles(0x1000, 0, 0x3000), 3) == -1 and b"view 1" in err(), name         # a null entry
        assert call(h3, 3, o=out + eb // 2) == -2 and b"aligned" in err(), name
        assert call(_handles(0x1000, 0x2000, 0x1000), 3) == -2 and b"two views" in err(), name  # one accumulator twice: before a handle is looked into
        assert call(None, 0) == -1, name                                                       # a null beats a bad count


@pytest.mark.parametrize("T", PRECISIONS)
def test_the_batched_feature_pass_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    fn = lib.rtw_accum_features_batch_f64 if T is np.float64 else lib.rtw_accum_features_batch_f32
    cams = _capi.make_cameras([rtw.t_default_cam(elem_type=T)] * 3, T)
    seeds = _capi.make_seeds([1, 2, 3], 3)
    dummy, out = C.c_void_p(0x1000), 0x200000
    err = lib.rtw_last_error

    def call(P, scene=dummy, cm=cams, n=3, sd=seeds, acc=DUMMIES, o=out):
        return fn(scene, cm, n, sd, C.byref(P) if P is not None else None, _handles(*acc) if acc is not None else None, C.c_void_p(o), None)

    P = _capi.make_params(96, 54, 64)
    assert call(None) == -1 and b"null" in err()
    assert call(P, scene=None) == -1 and call(P, cm=None) == -1 and call(P, acc=None) == -1 and call(P, o=0) == -1
    assert call(P, acc=(0x1000, 0x2000, 0)) == -1 and b"view 2" in err()
    assert call(P, n=0) == -2 and b"n_views" in err() and call(P, n=-1) == -2
    for bad, msg in _bad_params(_capi):                               # everything the single-view call refuses for `p`
        assert call(bad) == -2 and msg in err(), msg
    assert call(P, o=out + 8) == -2 and b"aligned" in err()
    assert call(_capi.make_params(2 ** 31 - 1, 2 ** 31 - 1, 4)) == -5
    assert call(P, acc=(0x1000, 0x1000, 0x2000)) == -2 and b"two views" in err()
    assert call(P, sd=None, acc=(0x1000, 0x1000, 0x2000)) == -2                                       # seeds may be null
    assert call(_capi.make_params(96, 54, 64, shard_index=0, shard_count=2), acc=(0x1000, 0, 0x2000)) == -1      # a null beats a bad parameter


@pytest.mark.parametrize("T", PRECISIONS)
def test_the_guided_batched_device_form_is_refused_without_a_device(lib, T):
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_guided_filter_batch_device_" + sfx)
    W, H, N = 5, 3, 3
    n_img, n_feat, n_noise, n_work = N * W * H * 3 * eb, N * W * H * 8 * eb, N * W * H * eb, N * lib.rtw_denoise_work_bytes(W, H, eb)
    img, feat, out, work, noise = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000       # never dereferenced
    err = lib.rtw_last_error

    def call(d=None, w=W, h=H, nv=N, i=img, f=feat, n=noise, o=out, k=work, none=False):
        d = _d() if d is None else d
        return fn(None if none else C.byref(d), w, h, nv, C.c_void_p(i), C.c_void_p(f), C.c_void_p(n), C.c_void_p(o), C.c_void_p(k), None)

    assert call(none=True) == -1 and b"null" in err()
    assert call(i=0) == -1 and call(f=0) == -1 and call(o=0) == -1 and call(k=0) == -1
    assert call(n=0) == -1 and b"null" in err()
    assert call(nv=0) == -2 and b"n_views" in err() and call(nv=-3) == -2
    for bad in BAD_DENOISE:
        assert call(_d(**bad)) == -2, bad
    assert call(w=0) == -2 and call(h=0) == -2 and call(w=2 ** 31 - 1, h=2 ** 31 - 1) == -5
    assert call(w=2 ** 15, h=2 ** 15, nv=2 ** 9) == -5 and b"batch too large" in err()     # 2^39 pixels
    assert call(k=work + 8) == -2 and b"aligned" in err()
    assert call(f=feat + 8) == -2 and call(i=img + 2) == -2 and call(o=out + 2) == -2
    assert call(n=noise + 2) == -2 and b"aligned" in err()
    # aliasing over the BATCH's extents: the last element of the last view still counts
    assert call(o=img) == -2 and b"alias" in err()
    assert call(o=feat + n_feat - eb) == -2 and call(o=work + n_work - eb) == -2 and call(k=img + n_img - eb) == -2
    assert call(o=noise + n_noise - eb) == -2 and b"alias" in err() and call(o=noise - n_img + eb) == -2
    assert call(k=noise + n_noise - eb) == -2 and b"alias" in err()
    assert call(_d(levels=0), n=0) == -1                               # a null beats a bad parameter
    if not _has_gpu():                                                 # (a call that passes every check is made only where nothing can launch)
        assert call() not in (0, -1, -2, -5)                           # everything in order: only the device is missing
        assert call(o=noise + n_noise) not in (0, -1, -2, -5)          # right behind the maps: no overlap


@pytest.mark.parametrize("T", PRECISIONS)
def test_the_batched_one_call_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    fn = lib.rtw_accum_filtered_batch_f64 if T is np.float64 else lib.rtw_accum_filtered_batch_f32
    cams = _capi.make_cameras([rtw.t_default_cam(elem_type=T)] * 3, T)
    seeds = _capi.make_seeds([1, 2, 3], 3)
    dummy = C.c_void_p(0x1000)
    out = np.zeros(3 * 96 * 54 * 3, T)
    err = lib.rtw_last_error

    def call(P, d=None, scene=dummy, cm=cams, n=3, sd=seeds, acc=DUMMIES, guided=1, o=out, no_d=False):
        d = _d() if d is None else d
        return fn(scene, cm, n, sd, C.byref(P) if P is not None else None, None if no_d else C.byref(d), _handles(*acc) if acc is not None else None, guided,
                  o.ctypes.data_as(C.c_void_p) if o is not None else None)

    P = _capi.make_params(96, 54, 64)
    assert call(None) == -1 and b"null" in err()
    assert call(P, scene=None) == -1 and call(P, cm=None) == -1 and call(P, acc=None) == -1 and call(P, o=None) == -1 and call(P, no_d=True) == -1
    assert call(P, acc=(0, 0x1000, 0x2000)) == -1 and b"view 0" in err()
    assert call(P, n=0) == -2 and b"n_views" in err() and call(P, n=-2) == -2
    assert call(P, guided=2) == -2 and b"guided" in err() and call(P, guided=-1) == -2
    for bad, msg in _bad_params(_capi):
        assert call(bad) == -2 and msg in err(), msg
        assert call(bad, guided=0) == -2
    for bad in BAD_DENOISE:
        assert call(P, _d(**bad)) == -2, bad
    assert call(_capi.make_params(2 ** 31 - 1, 2 ** 31 - 1, 4)) == -5
    assert call(P, acc=(0x1000, 0x2000, 0x2000)) == -2 and b"two views" in err()
    assert call(P, _d(levels=0), acc=(0x1000, 0, 0x2000)) == -1        # a null beats a bad parameter


def test_python_validation(rtw):
    with pytest.raises(ValueError):
        rtw.denoise_guided_batch_into(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 5, 3, 2, work_bytes=16)
    with pytest.raises(ValueError):
        rtw.denoise_guided_batch_into(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 5, 3, 0)
    with pytest.raises(TypeError):
        rtw.render_adaptive_denoised_batch(rtw.scene_2_spheres(elem_type=np.float32), ["camera"], 96, 4, tolerance=0.1)


def test_c_example_compiles_and_links(tmp_path):
    """examples/render_adaptive_denoised_batch_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_adaptive_denoised_batch_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "render_adaptive_denoised_batch_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "16", "3"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr


def test_unit_ops_30_and_31_validate_before_any_hip_call(lib):
    """the layouts of ops 30 / 31 (include/rtw_hip.h): nulls -> -1; a size or value they do not hold -> -2; 29 stays unknown, 36 is the first
    number behind the last op (32 - 35: the sinks with a flush counter, tests/test_gpu_list_caps.py)"""
    out = np.zeros(256, np.float64)
    head = np.zeros(8 + 2 * (1 + 8), np.float64)

    def unit(op, count, x, y, f32=False):
        f = lib.rtw_unit_f32 if f32 else lib.rtw_unit_f64
        return f(op, count, x.ctypes.data_as(C.c_void_p) if x is not None else None, y.ctypes.data_as(C.c_void_p) if y is not None else None, None, None)

    def call(op, f32=False, **kw):
        h = head.copy()
        h[:5] = [kw.get("width", 1), kw.get("height", 1), kw.get("spp", 4), kw.get("cs", 1), kw.get("slot4", 1 if op == 30 else 0.03)]
        h[5] = kw.get("pad", 0)
        h[8], h[8 + 9] = kw.get("chunks", 2), kw.get("chunks1", 3)         # two views of 1 x 1: C_t | 8 words each
        return unit(op, kw.get("count", 2), h, out, f32=f32)

    for op in (30, 31):
        assert unit(op, 2, None, out) == -1 and unit(op, 2, head, None, f32=True) == -1
        for bad in (dict(count=0), dict(count=-1), dict(width=0), dict(height=2 ** 15), dict(width=2048, height=1024), dict(spp=0), dict(cs=0), dict(cs=1.5),
                    dict(pad=1), dict(chunks=0), dict(chunks1=1.25), dict(slot4=float("nan")), dict(slot4=-1.0), dict(width=1024, height=1024, count=9)):
            assert call(op, **bad) == -2 and call(op, f32=True, **bad) == -2, (op, bad)
    assert call(30, slot4=2) == -2 and call(30, slot4=0.5) == -2 and call(31, slot4=float("inf")) == -2
    assert unit(29, 1, head, out) == -2 and b"unknown unit op" in lib.rtw_last_error()
    assert unit(36, 1, head, out) == -2 and b"unknown unit op" in lib.rtw_last_error()
    if not _has_gpu():
        for rc in (call(30), call(31), call(30, f32=True), call(31, f32=True)):
            assert rc > 0 or rc in (-21, -22), rc
            assert b"no HIP device" in lib.rtw_last_error()
