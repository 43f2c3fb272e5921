"""The progressive render's C ABI and Python helpers, CPU only (include/rtw_hip.h rtw_accum_*, rtw_render_accum_*): the symbols are
declared, listed and exported, every argument check the header promises for a pass is decided before any HIP call -- so these codes come
back without a device -- the chunk arithmetic of the Python mirror agrees with the library's rule, and a bad blob is refused."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ACCUM_SYMBOLS = ["rtw_accum_create", "rtw_accum_reset", "rtw_accum_free", "rtw_render_accum_f32", "rtw_render_accum_f64",
                 "rtw_accum_resolve_f32", "rtw_accum_resolve_f64", "rtw_accum_resolve_host_f32", "rtw_accum_resolve_host_f64",
                 "rtw_accum_merge", "rtw_accum_info", "rtw_accum_ranges", "rtw_accum_read_pixels", "rtw_accum_export", "rtw_accum_import"]


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


def test_accum_symbols_declared_exported_and_listed(lib):
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ACCUM_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert lib.rtw_abi_version() == 4


def _info_struct_matches_header():
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} rtw_accum_info_t;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip() for n in decl.split(None, 1)[1].split(",")]
    return names


def test_info_struct_mirrors_the_header():
    from rtw_amd import _capi
    assert [k for k, _ in _capi.AccumInfo._fields_] == _info_struct_matches_header()


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_pass_is_refused_without_a_device(lib, rtw, T):
    """nulls -> -1, the render's own checks and whole-frames-on-one-device -> -2, the chunk range -> -2: all before the handles are looked
    at (the dummy handles below are never dereferenced) and before any HIP call"""
    from rtw_amd import _capi
    fn = lib.rtw_render_accum_f64 if T is np.float64 else lib.rtw_render_accum_f32
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    dummy = C.c_void_p(0x1000)

    def call(P, begin=0, count=1, scene=dummy, cm=cam, acc=dummy):
        return fn(scene, C.byref(cm) if cm is not None else None, C.byref(P) if P is not None else None, begin, count, acc, None, None)

    P = _capi.make_params(96, 54, 16)
    assert call(None) == -1 and b"null" in lib.rtw_last_error()
    assert call(P, cm=None) == -1
    assert call(P, acc=None) == -1
    assert call(P, scene=None) == -1
    assert call(_capi.make_params(96, 54, 16, shard_index=0, shard_count=2)) == -2 and b"shard_count" in lib.rtw_last_error()
    assert call(_capi.make_params(96, 54, 16, flags=_capi.FLAG_COMPACT_TILES)) == -2 and b"COMPACT_TILES" in lib.rtw_last_error()
    assert call(_capi.make_params(96, 54, 16, flags=_capi.FLAG_RCCL_REDUCE)) == -2 and b"RCCL_REDUCE" in lib.rtw_last_error()
    assert call(_capi.make_params(96, 54, 16, flags=_capi.FLAG_RAY_POOL)) == -2 and b"RAY_POOL" in lib.rtw_last_error()
    assert call(_capi.make_params(96, 54, 16, devices=[0, 1])) == -2 and b"n_devices" in lib.rtw_last_error()
    assert call(_capi.make_params(96, 54, 16, devices=[0])) == -2 and b"device_ids" in lib.rtw_last_error()
    assert call(_capi.make_params(0, 54, 16)) == -2                       # the single render's checks too
    assert call(_capi.make_params(96, 54, 0)) == -2
    # the chunk range, in units of the EFFECTIVE chunks: 16 spp -> 16 chunks; 16 spp in 5 chunks -> chunk size 4 -> 4 chunks
    assert call(P, begin=-1) == -2 and b"chunk range" in lib.rtw_last_error()
    assert call(P, count=0) == -2
    assert call(P, begin=16, count=1) == -2
    assert call(P, begin=10, count=7) == -2
    assert call(P, begin=2**31 - 1, count=2**31 - 1) == -2
    assert call(_capi.make_params(96, 54, 16, n_chunks=5), begin=4, count=1) == -2 and b"4 chunks" in lib.rtw_last_error()
    assert call(_capi.make_params(96, 54, 16, n_chunks=40), begin=16, count=1) == -2      # (n_chunks > spp: spp chunks)
    # precedence: a bad render and a null handle -> the null is reported
    assert call(_capi.make_params(96, 54, 16, shard_index=0, shard_count=2), acc=None) == -1


def test_other_entry_points_refuse_nulls_without_a_device(lib):
    from rtw_amd import _capi
    dummy = C.c_void_p(0x1000)
    h = C.c_void_p()
    assert lib.rtw_accum_create(0, 96, 54, None) == -1
    assert lib.rtw_accum_create(0, 0, 54, C.byref(h)) == -2 and b"positive" in lib.rtw_last_error()
    assert lib.rtw_accum_create(0, 96, -1, C.byref(h)) == -2
    assert lib.rtw_accum_create(0, 1 << 20, 1 << 20, C.byref(h)) == -5 and b"too large" in lib.rtw_last_error()
    assert not h
    assert lib.rtw_accum_free(None) == 0
    assert lib.rtw_accum_reset(None, None) == -1
    assert lib.rtw_accum_merge(None, dummy, None) == -1 and lib.rtw_accum_merge(dummy, None, None) == -1
    assert lib.rtw_accum_merge(dummy, dummy, None) == -2
    assert lib.rtw_accum_info(None, C.byref(_capi.AccumInfo())) == -1 and lib.rtw_accum_info(dummy, None) == -1
    n = C.c_int32()
    assert lib.rtw_accum_ranges(None, 0, C.byref(n), None) == -1
    assert lib.rtw_accum_read_pixels(None, dummy) == -1 and lib.rtw_accum_read_pixels(dummy, None) == -1
    assert lib.rtw_accum_export(None, None, 0, C.byref(C.c_uint64())) == -1
    for fn in (lib.rtw_accum_resolve_f32, lib.rtw_accum_resolve_f64):
        assert fn(None, 1, dummy, None) == -1 and fn(dummy, 1, None, None) == -1
    for fn in (lib.rtw_accum_resolve_host_f32, lib.rtw_accum_resolve_host_f64):
        assert fn(None, 1, dummy) == -1 and fn(dummy, 1, None) == -1


def _params_rule(lib, spp, n_chunks):
    """the library's own effective chunk count, read off the pass's range check: the largest `begin` a one-chunk pass is not refused
    -2 for ... without a device every accepted range goes on to dereference a handle, so probe with the refusal message instead"""
    from rtw_amd import _capi
    P = _capi.make_params(8, 4, spp, n_chunks=n_chunks)
    cam = _capi.CameraF32()
    dummy = C.c_void_p(0x1000)
    assert lib.rtw_render_accum_f32(dummy, C.byref(cam), C.byref(P), 2**30, 1, dummy, None, None) == -2
    return int(re.search(rb"render's (\d+) chunks", lib.rtw_last_error()).group(1))


def test_samples_in_chunks_agrees_with_the_library(lib, rtw):
    from rtw_amd.progressive import effective_chunks
    for spp in (1, 2, 3, 7, 10, 16, 17, 64, 100, 255, 256, 257, 1000, 1001):
        for n_chunks in (0, 1, 2, 3, 5, 6, 7, 16, 40, 250, 256, 300, 2000):
            nch, cs = effective_chunks(spp, n_chunks)
            assert nch == _params_rule(lib, spp, n_chunks), (spp, n_chunks)
            assert (nch - 1) * cs < spp <= nch * cs
            assert effective_chunks(spp, nch) == (nch, cs)              # (what ProgressiveRenderer.load relies on)
            per_chunk = [rtw.samples_in_chunks(spp, n_chunks, c, 1) for c in range(nch)]
            assert sum(per_chunk) == spp and all(s == cs for s in per_chunk[:-1]) and 1 <= per_chunk[-1] <= cs
            assert rtw.samples_in_chunks(spp, n_chunks, 0, nch) == spp
            for b, c in ((0, 1), (nch // 2, nch - nch // 2), (nch - 1, 1)):
                assert rtw.samples_in_chunks(spp, n_chunks, b, c) == sum(per_chunk[b:b + c])
            with pytest.raises(ValueError):
                rtw.samples_in_chunks(spp, n_chunks, nch, 1)
            with pytest.raises(ValueError):
                rtw.samples_in_chunks(spp, n_chunks, 0, nch + 1)
    with pytest.raises(ValueError):
        rtw.samples_in_chunks(0, 0, 0, 1)
    with pytest.raises(ValueError):
        rtw.samples_in_chunks(4, 0, -1, 1)
    with pytest.raises(ValueError):
        rtw.samples_in_chunks(4, 0, 0, 0)


def _blob(width=2, height=1, version=1, n_ranges=0, bound=0):
    """a blob as rtw_accum_export writes it for an unbound accumulator (header 248 bytes: see rtw_accum.hip BlobHeader)"""
    head = b"RTWACCUM" + np.array([version, 248], np.uint32).tobytes() + np.array([width, height, bound, n_ranges], np.int32).tobytes()
    head += bytes(248 - len(head))
    return head + bytes(8 * n_ranges) + bytes(width * height * 64)


def test_import_refuses_bad_blobs_without_a_device(lib):
    h = C.c_void_p()

    def imp(b):
        buf = np.frombuffer(b, np.uint8)
        return lib.rtw_accum_import(0, buf.ctypes.data_as(C.c_void_p) if len(b) else C.c_void_p(0x1000), len(b), C.byref(h))

    good = _blob()
    assert imp(good[:-1]) == -2 and b"truncated" in lib.rtw_last_error()
    assert imp(good[:100]) == -2 and b"truncated" in lib.rtw_last_error()
    assert imp(b"") == -2
    assert imp(good + b"\0") == -2
    assert imp(_blob(version=2)) == -2 and b"version 2" in lib.rtw_last_error()
    assert imp(b"NOTACCUM" + good[8:]) == -2
    assert imp(_blob(width=0)) == -2
    assert imp(_blob(n_ranges=1)) == -2                 # ranges without a render
    assert lib.rtw_accum_import(0, None, 10, C.byref(h)) == -1
    assert not h
    if not _has_gpu():      # the well-formed blob gets as far as the device
        assert imp(good) > 0 or imp(good) in (-21, -22)
        assert b"no HIP device" in lib.rtw_last_error()


def test_python_validation(rtw):
    scene = rtw.scene_2_spheres(elem_type=np.float32)
    cam = rtw.t_default_cam(elem_type=np.float32)
    with pytest.raises(TypeError):
        rtw.ProgressiveRenderer(scene, "not a camera", 96, 4)
    with pytest.raises(ValueError):
        rtw.ProgressiveRenderer(scene, cam, 0, 4)
    with pytest.raises(ValueError):
        rtw.ProgressiveRenderer(scene, cam, 96, 0)
    with pytest.raises(ValueError):
        rtw.render_progressive(scene, cam, 96, 4, passes=0)
    for name in ("ProgressiveRenderer", "render_progressive", "samples_in_chunks"):
        assert name in rtw.__all__


def test_progressive_paths_do_not_import_torch():
    code = ("import sys, rtw_amd; from rtw_amd import progressive; "
            "assert 'torch' not in sys.modules, 'torch imported'")
    r = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_progressive_fails_loudly_without_gpu(rtw):
    from rtw_amd._capi import RtwError
    scene = rtw.scene_2_spheres(elem_type=np.float32)
    with pytest.raises(RtwError, match="no HIP device"):
        rtw.render_progressive(scene, rtw.t_default_cam(), 96, 4, passes=2)
    h = C.c_void_p()
    from rtw_amd import _capi
    assert _capi.lib().rtw_accum_create(0, 96, 54, C.byref(h)) != 0 and not h


def test_c_progressive_example_compiles_and_links(tmp_path):
    """examples/render_progressive_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_progressive_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "render_progressive_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "8", "4"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr
