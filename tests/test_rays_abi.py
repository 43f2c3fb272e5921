"""Ray queries, CPU only (include/rtw_hip.h rtw_cast_rays_*): the four symbols are declared, listed and exported, the parameter struct has
the size the header says, the header block names what is left out, and every refusal of both forms is decided before any HIP call (the
dummy device pointers below are never dereferenced; a bad parameter is refused before the handle is looked at)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_temporal_noise_abi import _has_gpu

RAYS_SYMBOLS = ["rtw_cast_rays_device_f32", "rtw_cast_rays_device_f64", "rtw_cast_rays_f32", "rtw_cast_rays_f64"]
PY_NAMES = ["cast_rays", "cast_rays_into", "make_rays_params"]
#: (field values, what the message names)
BAD_PARAMS = [(dict(flags=2), b"flags"), (dict(flags=8), b"flags"), (dict(flags=16), b"flags"), (dict(flags=64), b"flags"), (dict(flags=256), b"flags"),
              (dict(flags=32 | 128), b"exclude"), (dict(reserved=1), b"reserved"), (dict(device=-2), b"device"), (dict(max_workgroups=-1), b"max_workgroups"),
              (dict(tmin=-1e-4), b"tmin"), (dict(tmin=math.nan), b"tmin"), (dict(tmin=math.inf), b"tmin")]
GOOD_FLAGS = [0, 1, 4, 5, 32, 128, 1 | 4 | 128]


@pytest.fixture(scope="module")
def lib(rtw):
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def _p(**kw):
    from rtw_amd import _capi
    P = _capi.RaysParams(0, -1, 0, 0, 1e-4)
    for k, v in kw.items():
        setattr(P, k, v)
    return P


def test_symbols_declared_exported_and_listed(lib, rtw):
    import inspect
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in RAYS_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert sorted(n for n in declared if "cast_rays" in n) == sorted(RAYS_SYMBOLS)
    assert lib.rtw_abi_version() == 4                    # additive: the ABI version stays
    assert C.sizeof(_capi.RaysParams) == 24 and "} rtw_rays_params;" in header
    assert [f[0] for f in _capi.RaysParams._fields_] == ["flags", "device", "max_workgroups", "reserved", "tmin"] and _capi.RaysParams.tmin.offset == 16
    for name in PY_NAMES:
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name
    assert list(inspect.signature(rtw.DeviceRenderer.cast_rays_into).parameters)[:5] == ["self", "d_rays_ptr", "n", "d_idx_ptr", "d_rec_ptr"]
    assert {"tmin", "T", "flags", "stream", "max_workgroups"} <= set(inspect.signature(rtw.cast_rays_into).parameters)
    block = header[header.index("Ray queries: the closest hit"):header.index("rtw_cast_rays_device_f32(")]
    for word in ("Left out on purpose", "any-hit", "group cull on caller rays", "tmin per ray", "scatter and shading", "device lists", "the Julia shim",
                 "LATER of two spheres", "all +0 on a miss"):
        assert word in block, word


def test_the_struct_in_c_has_24_bytes(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include "rtw_hip.h"\n#include <stddef.h>\n'
                   'int main(void) { return sizeof(rtw_rays_params) == 24 && offsetof(rtw_rays_params, tmin) == 16 && offsetof(rtw_rays_params, reserved) == 12 ? 0 : 1; }\n')
    exe = str(tmp_path / "size")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([exe]).returncode == 0


def test_make_rays_params_and_pack_rays(rtw):
    from rtw_amd import _capi
    from rtw_amd.rays import pack_rays
    P = rtw.make_rays_params(tmin=0.5, flags=4, max_workgroups=3, numerics="contract")
    assert (P.flags, P.device, P.max_workgroups, P.reserved, P.tmin) == (4 | _capi.FLAG_NUMERICS_CONTRACT, -1, 3, 0, 0.5)
    with pytest.raises(ValueError):
        rtw.make_rays_params(flags=_capi.FLAG_NUMERICS_CONTRACT, numerics="reference_fma2")
    r6 = np.arange(12.0).reshape(2, 6)
    p = pack_rays(r6, np.float32)
    assert p.dtype == np.float32 and p.shape == (2, 8) and np.array_equal(p[:, :6], r6) and np.isposinf(p[:, 6]).all() and (p[:, 7] == 0).all()
    r7 = np.arange(14.0).reshape(2, 7)
    p = pack_rays(r7, np.float64)
    assert p.dtype == np.float64 and np.array_equal(p[:, :7], r7) and (p[:, 7] == 0).all()
    assert np.array_equal(pack_rays(np.arange(16.0).reshape(2, 8), np.float64), np.arange(16.0).reshape(2, 8))
    with pytest.raises(ValueError):
        pack_rays(np.zeros((2, 5)))


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_device_form_is_refused_without_a_device(lib, T):
    sfx = "f64" if T is np.float64 else "f32"
    dev = getattr(lib, "rtw_cast_rays_device_" + sfx)
    err = lib.rtw_last_error
    handle, rays, idx, rec = 0x100000, 0x200000, 0x300000, 0x400000       # never dereferenced: every refusal below comes before the handle is looked at
    vp = lambda x: C.c_void_p(x) if x else None

    def call(p=None, s=handle, r=rays, n=100, i=idx, o=rec, none=None):
        p = _p() if p is None else p
        return dev(vp(s), vp(r), n, None if none == "p" else C.byref(p), vp(i), vp(o), None)

    assert call(none="p") == -1 and b"null" in err() and call(s=0) == -1 and call(r=0) == -1 and call(i=0) == -1
    assert call(_p(flags=2), s=0) == -1                   # precedence: a null beats a bad parameter
    for bad, word in BAD_PARAMS:
        assert call(_p(**bad)) == -2 and word in err(), bad
        assert call(_p(**bad), o=0) == -2, bad
    assert call(n=-1) == -2 and b"ray count" in err() and call(n=-2 ** 40) == -2
    assert call(n=2 ** 31) == -5 and call(n=2 ** 40) == -5 and call(_p(flags=2), n=2 ** 31) == -2
    assert call(r=rays + 8) == -2 and b"aligned" in err() and call(o=rec + 8) == -2 and call(r=rays + 4) == -2
    assert call(i=idx + 2) == -2 and b"4-byte" in err() and call(i=idx + 1) == -2


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_host_form_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    host = getattr(lib, "rtw_cast_rays_" + sfx)
    err = lib.rtw_last_error
    flat = rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T)
    S, keep = _capi.make_scene(flat, T)
    n = 10
    rays, idx, rec = np.zeros((n, 8), T), np.zeros(n, np.int32), np.zeros((n, 8), T)
    rays[:, 5], rays[:, 6] = -1.0, np.inf
    vp = lambda x: C.c_void_p(x) if x else None

    def call(p=None, s=S, r=rays.ctypes.data, n=n, i=idx.ctypes.data, o=rec.ctypes.data):
        return host(None if s is None else C.byref(s), vp(r), n, None if p == "null" else C.byref(_p() if p is None else p), vp(i), vp(o))

    assert call(p="null") == -1 and b"null" in err() and call(s=None) == -1 and call(r=0) == -1 and call(i=0) == -1
    for bad, word in BAD_PARAMS:
        assert call(_p(**bad)) == -2 and word in err(), bad
    assert call(n=-1) == -2 and call(n=2 ** 31) == -5
    # host buffers that overlap: the first offending pair is named -- the outputs against each other, then against the rays
    assert call(o=idx.ctypes.data) == -2 and b"idx and rec may not alias each other" in err()
    assert call(i=rays.ctypes.data + 16) == -2 and b"idx may not alias the rays" in err()
    assert call(o=rays.ctypes.data + n * 8 * eb - eb) == -2 and b"rec may not alias the rays" in err()
    assert call(i=rec.ctypes.data, o=rec.ctypes.data) == -2 and b"idx and rec" in err()
    bad = type(S)()
    C.memmove(C.byref(bad), C.byref(S), C.sizeof(S))
    bad.n = -1
    assert call(s=bad) == -2 and b"sphere count" in err()
    bad.n = 2
    bad.r = None
    assert call(s=bad) == -1 and b"scene array" in err()
    # n == 0: nothing to do, on a machine without a GPU too; the parameters are still checked
    assert call(n=0) == 0 and call(n=0, o=0) == 0 and call(_p(flags=2), n=0) == -2
    assert rtw.cast_rays(flat, np.zeros((0, 6)), T=T)[0].shape == (0,)
    if not _has_gpu():
        for flags in GOOD_FLAGS:
            assert call(_p(flags=flags)) not in (0, -1, -2, -4, -5), flags      # everything in order: only the device is missing
        assert call(o=0) not in (0, -1, -2, -4, -5) and call(_p(tmin=0.0, max_workgroups=7)) not in (0, -1, -2, -4, -5)
    del keep


def test_c_example_compiles_and_links(tmp_path):
    """examples/cast_rays_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "cast_rays_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "cast_rays_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr
