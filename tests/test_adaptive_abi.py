"""Adaptive sampling, CPU only (include/rtw_hip.h rtw_render_adaptive_*, rtw_accum_adaptive_info, rtw_accum_tile_chunks): the symbols are
declared, listed and exported; every refusal that needs no accumulator is decided before any HIP call and before a handle is looked at
(the refusals that need a real accumulator -- -4 for a binding, -2 for plain passes / merge / export on an adaptive accumulator -- are in
tests/test_gpu_adaptive.py, next to the check that they leave the accumulator unchanged); and the Python restatement of the stopping rule,
the witness of the GPU tests, is checked against hand-made accumulator words."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ADAPTIVE_SYMBOLS = ["rtw_render_adaptive_f32", "rtw_render_adaptive_f64", "rtw_accum_adaptive_info", "rtw_accum_tile_chunks"]


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


def test_adaptive_symbols_declared_exported_and_listed(lib):
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ADAPTIVE_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert lib.rtw_abi_version() == 4                    # additive: the ABI version stays


def _struct_fields(header, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*\]", "", n).strip() for n in decl.split(None, 1)[1].split(",")]
    return names


def test_structs_mirror_the_header():
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    assert [k for k, _ in _capi.Adaptive._fields_] == _struct_fields(header, "rtw_adaptive_t")
    assert [k for k, _ in _capi.AdaptiveInfo._fields_] == _struct_fields(header, "rtw_adaptive_info_t")
    assert C.sizeof(_capi.Adaptive) == 32 and C.sizeof(_capi.AdaptiveInfo) == 40


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_an_adaptive_render_is_refused_without_a_device(lib, rtw, T):
    """nulls -> -1; the render's own checks, whole frames on one device and the adaptive parameters -> -2: all before the handles are
    looked at (the dummy handles below are never dereferenced) and before any HIP call"""
    from rtw_amd import _capi
    fn = lib.rtw_render_adaptive_f64 if T is np.float64 else lib.rtw_render_adaptive_f32
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    dummy = C.c_void_p(0x1000)
    good = _capi.Adaptive(0.05, 0.03, 0, 0)
    err = lib.rtw_last_error

    def call(P, A=good, scene=dummy, cm=cam, acc=dummy):
        return fn(scene, C.byref(cm) if cm is not None else None, C.byref(P) if P is not None else None,
                  C.byref(A) if A is not None else None, acc, None, None)

    P = _capi.make_params(96, 54, 64)
    assert call(None) == -1 and b"null" in err()
    assert call(P, A=None) == -1 and call(P, cm=None) == -1 and call(P, acc=None) == -1 and call(P, scene=None) == -1
    # the restrictions of rtw_render_accum_*
    assert call(_capi.make_params(96, 54, 64, shard_index=0, shard_count=2)) == -2 and b"shard_count" in err()
    assert call(_capi.make_params(96, 54, 64, flags=_capi.FLAG_COMPACT_TILES)) == -2 and b"COMPACT_TILES" in err()
    assert call(_capi.make_params(96, 54, 64, flags=_capi.FLAG_RCCL_REDUCE)) == -2 and b"RCCL_REDUCE" in err()
    assert call(_capi.make_params(96, 54, 64, flags=_capi.FLAG_RAY_POOL)) == -2 and b"RAY_POOL" in err()
    assert call(_capi.make_params(96, 54, 64, devices=[0, 1])) == -2 and b"n_devices" in err()
    assert call(_capi.make_params(96, 54, 64, devices=[0])) == -2 and b"device_ids" in err()
    assert call(_capi.make_params(0, 54, 64)) == -2 and call(_capi.make_params(96, 54, 0)) == -2
    # the adaptive parameters
    for tol in (0.0, -0.1, float("nan"), float("inf"), -float("inf")):
        assert call(P, A=_capi.Adaptive(tol, 0.03, 0, 0)) == -2 and b"tolerance" in err(), tol
    for floor in (-1e-9, float("nan"), float("inf")):
        assert call(P, A=_capi.Adaptive(0.05, floor, 0, 0)) == -2 and b"dark_floor" in err(), floor
    for bad in (1, 3, 17, -2, -1):
        assert call(P, A=_capi.Adaptive(0.05, 0.03, bad, 0)) == -2 and b"min_chunks" in err(), bad
        assert call(P, A=_capi.Adaptive(0.05, 0.03, 0, bad)) == -2 and b"check_chunks" in err(), bad
    # precedence: a bad render or bad parameters and a null handle -> the null is reported
    assert call(_capi.make_params(96, 54, 64, shard_index=0, shard_count=2), acc=None) == -1
    assert call(P, A=_capi.Adaptive(-1.0, 0.03, 0, 0), scene=None) == -1


def test_info_entry_points_refuse_nulls_without_a_device(lib):
    from rtw_amd import _capi
    dummy = C.c_void_p(0x1000)
    n = C.c_int32()
    assert lib.rtw_accum_adaptive_info(None, C.byref(_capi.AdaptiveInfo())) == -1 and lib.rtw_accum_adaptive_info(dummy, None) == -1
    assert lib.rtw_accum_tile_chunks(None, 0, C.byref(n), None) == -1 and lib.rtw_accum_tile_chunks(dummy, 0, None, None) == -1
    assert lib.rtw_accum_tile_chunks(dummy, 4, C.byref(n), None) == -1 and lib.rtw_accum_tile_chunks(dummy, -1, C.byref(n), None) == -1


# ---- reference_decisions against hand-made words -----------------------------------------------------------------------------------
def _words(width, height):
    return np.zeros((height, width, 8), np.uint64)


def _set(w, i, j, rgb=(0.0, 0.0, 0.0), h=0, poison=0):
    """pixel (i, j) (0-based): channel sums rgb (multiples of 2^-32, so exact), half difference h (units of 2^-24), poison count"""
    for c, v in enumerate(rgb):
        fx = int(round(v * 2 ** 32)) << 32
        assert fx / 2 ** 64 == v
        fx &= (1 << 128) - 1
        w[i, j, 2 * c], w[i, j, 2 * c + 1] = fx & (2 ** 64 - 1), fx >> 64
    w[i, j, 6], w[i, j, 7] = poison, h & (2 ** 64 - 1)


def test_reference_decisions_on_hand_made_words(rtw):
    rd = rtw.reference_decisions
    n = 10
    # 16 x 8: two tiles down one column.  Tile 0: every pixel alike, the halves agree (H = 0) -> converged at any tolerance
    w = _words(8, 16)
    for i in range(16):
        for j in range(8):
            _set(w, i, j, rgb=(1.0, 2.0, 3.0))
    # tile 1: the same sums, ONE pixel with a large half difference: |H| = 100 (in radiance) of a tile sum Y = 64 * 6 = 384
    _set(w, 8 + 3, 5, rgb=(1.0, 2.0, 3.0), h=-(100 << 24))
    conv, D, Y, M = rd(w, 8, 16, n, 0.25, 0.0, return_terms=True)
    assert list(conv) == [True, False]
    assert D == [0.0, 100.0] and Y == [384.0, 384.0] and M == [384.0, 384.0]
    assert list(rd(w, 8, 16, n, 100.0 / 384.0, 0.0)) == [True, True]          # D <= tol * M holds with equality
    assert list(rd(w, 8, 16, n, 0.26, 0.0)) == [True, False]                  # 0.26 * 384 = 99.84 < 100
    assert list(rd(w, 8, 16, n, 0.27, 0.0)) == [True, True]
    # the dark floor: floor * n * npix = 1 * 10 * 64 = 640 > Y -> D = 100 is judged against 640
    conv, D, Y, M = rd(w, 8, 16, n, 0.2, 1.0, return_terms=True)
    assert M == [640.0, 640.0] and list(conv) == [True, True]
    assert list(rd(w, 8, 16, n, 0.15, 1.0)) == [True, False]
    # a poisoned pixel is ignored: poisoning the noisy pixel takes its H AND its sums out
    _set(w, 8 + 3, 5, rgb=(1.0, 2.0, 3.0), h=-(100 << 24), poison=2)
    conv, D, Y, M = rd(w, 8, 16, n, 1e-6, 0.0, return_terms=True)
    assert list(conv) == [True, True] and D == [0.0, 0.0] and Y == [384.0, 378.0]
    # ... and still counts as a pixel of the tile in the dark floor's npix
    assert rd(w, 8, 16, n, 1.0, 1.0, return_terms=True)[3] == [640.0, 640.0]
    # negative channel sums: y_p is clamped at 0 per pixel
    _set(w, 0, 0, rgb=(-4.0, 1.0, 1.0))
    assert rd(w, 8, 16, n, 1.0, 0.0, return_terms=True)[2][0] == 384.0 - 6.0
    # a ragged frame 11 x 13 (W x H): tiles of 8x8, 5x8 (last rows), 8x3 (last columns), 5x3 valid pixels, numbered column-major
    w = _words(11, 13)
    for i in range(13):
        for j in range(11):
            _set(w, i, j, rgb=(0.5, 0.0, 0.0), h=1 << 23)                      # |H| = 0.5 per pixel: D = npix / 2 = Y
    conv, D, Y, M = rd(w, 11, 13, n, 1.0, 0.1, return_terms=True)
    npix = [64, 40, 24, 15]
    assert D == [p * 0.5 for p in npix] and Y == D and M == [0.1 * 10 * p for p in npix]      # floor * n * npix with each tile's OWN npix
    assert list(conv) == [True] * 4 and not rd(w, 11, 13, n, 0.49, 0.1).any()
    # the order of the operations: (floor * n) * npix, rounded after each step
    assert rd(w, 11, 13, 3, 1.0, 1.3, return_terms=True)[3][3] == (1.3 * 3.0) * 15.0 == 58.50000000000001 != 1.3 * (3.0 * 15.0)


def test_checkpoints_and_defaults(rtw):
    from rtw_amd import adaptive
    assert adaptive.default_check_chunks(64) == 16 and adaptive.default_check_chunks(250) == 32 and adaptive.default_check_chunks(256) == 32
    assert adaptive.default_check_chunks(130) == 18 and adaptive.default_check_chunks(1) == 16
    assert adaptive.checkpoints(64) == [16, 32, 48] and adaptive.checkpoints(250) == [32, 64, 96, 128, 160, 192, 224]
    assert adaptive.checkpoints(8) == [] and adaptive.checkpoints(8, 2, 4) == [2, 6] and adaptive.checkpoints(16) == []
    assert adaptive.noise_q(1.0) == 1 << 24 and adaptive.noise_q(64.0) == 2 ** 30 - 1 and adaptive.noise_q(1e9) == 2 ** 30 - 1
    assert adaptive.noise_q(-1.0) == 0 and adaptive.noise_q(float("nan")) == 0 and adaptive.noise_q(3e9) == 0 and adaptive.noise_q(2.0 ** -25) == 0
    assert adaptive.noise_q(0.75 + 2.0 ** -30) == 3 << 22
    for name in ("AdaptiveRenderer", "render_adaptive", "reference_decisions"):
        assert name in rtw.__all__


def test_python_validation(rtw):
    scene = rtw.scene_2_spheres(elem_type=np.float32)
    cam = rtw.t_default_cam(elem_type=np.float32)
    with pytest.raises(TypeError):
        rtw.AdaptiveRenderer(scene, "not a camera", 96, 4)
    with pytest.raises(ValueError):
        rtw.AdaptiveRenderer(scene, cam, 96, 0)
    with pytest.raises(TypeError):
        rtw.render_adaptive(scene, cam, 96, 4)             # tolerance is required


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_adaptive_fails_loudly_without_gpu(rtw):
    from rtw_amd._capi import RtwError
    scene = rtw.scene_2_spheres(elem_type=np.float32)
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.render_adaptive(scene, rtw.t_default_cam(), 96, 4, tolerance=0.05)


def test_c_adaptive_example_compiles_and_links(tmp_path):
    """examples/render_adaptive_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_adaptive_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "render_adaptive_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "32", "0.05"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr
