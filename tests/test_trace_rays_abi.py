"""Radiance queries, CPU only (include/rtw_hip.h rtw_trace_rays_*): the four symbols are declared, listed and exported, the parameter
struct has the size and the offsets the header says, the header block states the definition's consequences and what is left out, and
every refusal of both forms is decided before any HIP call (the dummy device pointers below are never dereferenced; a bad parameter is
refused before the handle is looked at)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_temporal_noise_abi import _has_gpu

TRACE_SYMBOLS = ["rtw_trace_rays_device_f32", "rtw_trace_rays_device_f64", "rtw_trace_rays_f32", "rtw_trace_rays_f64"]
PY_NAMES = ["trace_rays", "trace_rays_into", "make_trace_params"]
FIELDS = ["flags", "device", "max_workgroups", "spp", "max_depth", "reserved", "seed", "first_stream", "first_sample"]
OFFSETS = [0, 4, 8, 12, 16, 20, 24, 32, 40]
U64 = 2 ** 64
#: (field values, what the message names)
BAD_PARAMS = [(dict(flags=2), b"flags"), (dict(flags=8), b"flags"), (dict(flags=16), b"flags"), (dict(flags=64), b"flags"), (dict(flags=256), b"flags"),
              (dict(flags=32 | 128), b"exclude"), (dict(reserved=1), b"reserved"), (dict(device=-2), b"device"), (dict(max_workgroups=-1), b"max_workgroups"),
              (dict(spp=0), b"spp"), (dict(spp=-3), b"spp"), (dict(max_depth=-1), b"max_depth"), (dict(max_depth=1 << 22), b"max_depth"),
              (dict(first_stream=U64 - 9), b"first_stream"), (dict(first_stream=U64 - 1), b"first_stream"),
              (dict(first_sample=U64 - 4, spp=4), b"first_sample"), (dict(first_sample=U64 - 1, spp=2), b"first_sample")]
GOOD_PARAMS = [dict(flags=f) for f in (0, 1, 4, 5, 32, 128, 1 | 4 | 128)] + [dict(max_depth=0), dict(max_depth=(1 << 22) - 1), dict(spp=2 ** 31 - 1),
                                                                             dict(first_stream=U64 - 100), dict(first_sample=U64 - 5, spp=4), dict(seed=U64 - 1)]


@pytest.fixture(scope="module")
def lib(rtw):
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def _p(**kw):
    from rtw_amd import _capi
    P = _capi.TraceParams(0, -1, 0, 1, 16, 0, 1, 0, 0)
    for k, v in kw.items():
        setattr(P, k, v)
    return P


def test_symbols_declared_exported_and_listed(lib, rtw):
    import inspect
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in TRACE_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert sorted(n for n in declared if "trace_rays" in n) == sorted(TRACE_SYMBOLS)
    assert lib.rtw_abi_version() == _capi.ABI_VERSION == 4                    # additive: the ABI version stays
    assert C.sizeof(_capi.TraceParams) == 48 and "} rtw_trace_params;           /* 48 bytes */" in header
    assert [f[0] for f in _capi.TraceParams._fields_] == FIELDS
    assert [getattr(_capi.TraceParams, f).offset for f in FIELDS] == OFFSETS
    for name in PY_NAMES:
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name
    assert list(inspect.signature(rtw.DeviceRenderer.trace_rays_into).parameters)[:4] == ["self", "d_rays_ptr", "n", "d_out_ptr"]
    sig = inspect.signature(rtw.trace_rays).parameters
    assert list(sig)[:2] == ["scene", "rays"] and sig["spp"].default is inspect.Parameter.empty and sig["spp"].kind is inspect.Parameter.KEYWORD_ONLY
    assert (sig["max_depth"].default, sig["seed"].default, sig["first_stream"].default, sig["first_sample"].default) == (16, 1, 0, 0)
    assert {"spp", "max_depth", "seed", "first_stream", "first_sample", "T", "flags", "stream", "max_workgroups"} <= set(inspect.signature(rtw.trace_rays_into).parameters)
    # the block stands behind the ray-query declarations and states the contract the tests use
    assert header.index("Radiance queries: ray_color") > header.index("int rtw_cast_rays_f64(")
    block = header[header.index("Radiance queries: ray_color"):header.index("int rtw_trace_rays_device_f32(")]
    text = re.sub(r"\s*\n \*\s*", " ", block)           # the comment as running text
    for word in ("One stream per SAMPLE", "No camera draw", "Elements 6 and 7 are not read", "64.64 fixed point", "divided by (double)spp", "n x 3 binary64",
                 "makes all three values of that ray NaN", "gives the words of the one call", "two independent estimates", "Left out on purpose",
                 "samples split across lanes", "group cull on caller rays", "tmin or tmax per ray", "resumable passes", "device lists", "the Julia shim",
                 "Additive to ABI 4"):
        assert word in text, word
    # no new flag constant (tests/test_host_abi.py pins the set): the block names existing ones only
    assert set(re.findall(r"RTW_FLAG_[A-Z0-9_]+", block)) <= {"RTW_FLAG_SCAN_VALU", "RTW_FLAG_GROUP_CULL", "RTW_FLAG_NUMERICS_"}


def test_the_struct_in_c_has_48_bytes(tmp_path):
    src = tmp_path / "size.c"
    offs = " && ".join(f"offsetof(rtw_trace_params, {f}) == {o}" for f, o in zip(FIELDS, OFFSETS))
    src.write_text('#include "rtw_hip.h"\n#include <stddef.h>\n'
                   f'int main(void) {{ return sizeof(rtw_trace_params) == 48 && {offs} ? 0 : 1; }}\n')
    exe = str(tmp_path / "size")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([exe]).returncode == 0


def test_make_trace_params(rtw):
    from rtw_amd import _capi
    P = rtw.make_trace_params(spp=7, max_depth=50, seed=U64 - 1, first_stream=2 ** 40, first_sample=3, flags=4, max_workgroups=3, numerics="contract")
    assert [getattr(P, f) for f in FIELDS] == [4 | _capi.FLAG_NUMERICS_CONTRACT, -1, 3, 7, 50, 0, U64 - 1, 2 ** 40, 3]
    P = rtw.make_trace_params(spp=1)
    assert [getattr(P, f) for f in FIELDS][3:] == [1, 16, 0, 1, 0, 0]
    with pytest.raises(ValueError):
        rtw.make_trace_params(spp=1, flags=_capi.FLAG_NUMERICS_CONTRACT, numerics="reference_fma2")
    with pytest.raises(TypeError):
        rtw.make_trace_params()


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_device_form_is_refused_without_a_device(lib, T):
    sfx = "f64" if T is np.float64 else "f32"
    dev = getattr(lib, "rtw_trace_rays_device_" + sfx)
    err = lib.rtw_last_error
    handle, rays, out = 0x100000, 0x200000, 0x300000       # never dereferenced: every refusal below comes before the handle is looked at
    vp = lambda x: C.c_void_p(x) if x else None

    def call(p=None, s=handle, r=rays, n=100, o=out, none=None):
        p = _p() if p is None else p
        return dev(vp(s), vp(r), n, None if none == "p" else C.byref(p), vp(o), None)

    assert call(none="p") == -1 and b"null" in err() and call(s=0) == -1 and call(r=0) == -1 and call(o=0) == -1
    assert call(_p(flags=2), s=0) == -1                   # precedence: a null beats a bad parameter
    for bad, word in BAD_PARAMS:
        assert call(_p(**bad)) == -2 and word in err(), bad
    assert call(n=-1) == -2 and b"ray count" in err() and call(n=-2 ** 40) == -2
    assert call(n=2 ** 31) == -5 and call(n=2 ** 40) == -5 and call(_p(flags=2), n=2 ** 31) == -2
    assert call(_p(first_stream=U64 - 100), n=101) == -2 and b"first_stream" in err()
    assert call(r=rays + 8) == -2 and b"16-byte" in err() and call(r=rays + 4) == -2
    assert call(o=out + 4) == -2 and b"8-byte" in err() and call(o=out + 1) == -2


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_host_form_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    host = getattr(lib, "rtw_trace_rays_" + sfx)
    err = lib.rtw_last_error
    flat = rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T)
    S, keep = _capi.make_scene(flat, T)
    n = 10
    rays, out = np.zeros((n, 8), T), np.zeros((n, 3), np.float64)
    rays[:, 5], rays[:, 6] = -1.0, np.inf
    vp = lambda x: C.c_void_p(x) if x else None

    def call(p=None, s=S, r=rays.ctypes.data, n=n, o=out.ctypes.data):
        return host(None if s is None else C.byref(s), vp(r), n, None if p == "null" else C.byref(_p() if p is None else p), vp(o))

    assert call(p="null") == -1 and b"null" in err() and call(s=None) == -1 and call(r=0) == -1 and call(o=0) == -1
    for bad, word in BAD_PARAMS:
        assert call(_p(**bad)) == -2 and word in err(), bad
    assert call(n=-1) == -2 and call(n=2 ** 31) == -5
    assert call(_p(first_stream=U64 - 10)) == -2 and b"first_stream" in err()        # first_stream + n = 2^64
    # host buffers that overlap: out against the rays, on their first and on their last byte
    assert call(o=rays.ctypes.data) == -2 and b"out may not alias the rays" in err()
    assert call(o=rays.ctypes.data + n * 8 * eb - 8) == -2 and b"out may not alias the rays" in err()
    assert call(r=out.ctypes.data + n * 24 - 16) == -2 and b"alias" in err()
    bad = type(S)()
    C.memmove(C.byref(bad), C.byref(S), C.sizeof(S))
    bad.n = -1
    assert call(s=bad) == -2 and b"sphere count" in err()
    bad.n = 2
    bad.r = None
    assert call(s=bad) == -1 and b"scene array" in err()
    # n == 0: nothing to do, on a machine without a GPU too; the parameters are still checked
    assert call(n=0) == 0 and call(_p(first_stream=U64 - 1), n=0) == 0 and call(_p(flags=2), n=0) == -2 and call(_p(spp=0), n=0) == -2
    assert rtw.trace_rays(flat, np.zeros((0, 6)), spp=4, T=T).shape == (0, 3)
    if not _has_gpu():
        for good in GOOD_PARAMS:
            assert call(_p(**good)) not in (0, -1, -2, -4, -5), good      # everything in order: only the device is missing
    del keep


def test_c_example_compiles_and_links(tmp_path):
    """examples/trace_rays_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "trace_rays_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "trace_rays_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr
