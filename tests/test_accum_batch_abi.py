"""Batched progressive and adaptive renders, CPU only (include/rtw_hip.h rtw_render_accum_batch_*, rtw_render_adaptive_batch_*): the four
symbols are declared, listed and exported, and every refusal that needs no real handle is decided before any HIP call and before a handle
is looked at (the dummy handles below are never dereferenced).  The refusals that need real accumulators -- a wrong size, a binding, a mix
of bound and unbound, a looser tolerance, a progressive batch on an adaptive accumulator -- are in tests/test_gpu_accum_batch.py, next to
the check that they leave every accumulator of the array unchanged."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

BATCH_SYMBOLS = ["rtw_render_accum_batch_f32", "rtw_render_accum_batch_f64", "rtw_render_adaptive_batch_f32", "rtw_render_adaptive_batch_f64"]


@pytest.fixture(scope="module")
def lib(rtw):
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def test_batch_symbols_declared_exported_and_listed(lib):
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in BATCH_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert lib.rtw_abi_version() == 4                    # additive: the ABI version stays


class _Calls:
    """both entry points of one precision with dummy scene / accumulator handles: n views of one camera"""

    def __init__(self, lib, rtw, T, n=3):
        from rtw_amd import _capi
        self.C, self.lib, self.n = _capi, lib, n
        f64 = T is np.float64
        self.accum_fn = lib.rtw_render_accum_batch_f64 if f64 else lib.rtw_render_accum_batch_f32
        self.adapt_fn = lib.rtw_render_adaptive_batch_f64 if f64 else lib.rtw_render_adaptive_batch_f32
        self.cams = _capi.make_cameras([rtw.t_default_cam(elem_type=T)] * n, T)
        self.scene = C.c_void_p(0x1000)
        self.accs = _capi.make_handles([0x2000 + 0x100 * k for k in range(n)])
        self.good = _capi.Adaptive(0.05, 0.03, 0, 0)

    def accum(self, P, begin=0, count=1, **kw):
        a = dict(scene=self.scene, cams=self.cams, n=self.n, accs=self.accs)
        a.update(kw)
        return self.accum_fn(a["scene"], a["cams"], a["n"], None, C.byref(P) if P is not None else None, begin, count, a["accs"], None, None)

    def adapt(self, P, A="good", **kw):
        a = dict(scene=self.scene, cams=self.cams, n=self.n, accs=self.accs)
        a.update(kw)
        A = self.good if A == "good" else A
        return self.adapt_fn(a["scene"], a["cams"], a["n"], None, C.byref(P) if P is not None else None, C.byref(A) if A is not None else None,
                             a["accs"], None, None)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_batched_passes_are_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    k = _Calls(lib, rtw, T)
    err = lib.rtw_last_error
    P = _capi.make_params(96, 54, 64)
    for call in (k.accum, k.adapt):
        # nulls, a null entry of accums
        assert call(None) == -1 and b"null" in err()
        assert call(P, scene=None) == -1 and call(P, cams=None) == -1 and call(P, accs=None) == -1
        assert call(P, accs=_capi.make_handles([0x2000, 0, 0x2200])) == -1 and b"view 1" in err()
        # n_views
        assert call(P, n=0) == -2 and b"n_views" in err()
        assert call(P, n=-3) == -2
        # the whole-frame, one-device restrictions of rtw_render_batch_* and rtw_render_accum_*
        assert call(_capi.make_params(96, 54, 64, shard_index=0, shard_count=2)) == -2 and b"shard_count" in err()
        assert call(_capi.make_params(96, 54, 64, flags=_capi.FLAG_COMPACT_TILES)) == -2 and b"COMPACT_TILES" in err()
        assert call(_capi.make_params(96, 54, 64, flags=_capi.FLAG_RCCL_REDUCE)) == -2 and b"RCCL_REDUCE" in err()
        assert call(_capi.make_params(96, 54, 64, flags=_capi.FLAG_RAY_POOL)) == -2 and b"RAY_POOL" in err()
        assert call(_capi.make_params(96, 54, 64, devices=[0, 1])) == -2 and b"n_devices" in err()
        assert call(_capi.make_params(96, 54, 64, devices=[0])) == -2 and b"device_ids" in err()
        assert call(_capi.make_params(0, 54, 64)) == -2 and call(_capi.make_params(96, 54, 0)) == -2
        # one accumulator twice in the array
        assert call(P, accs=_capi.make_handles([0x2000, 0x2100, 0x2000])) == -2 and b"two views" in err()
    # validate_batch's queue limit: 8 views of 32768 x 1024 tiles are 2^28 tiles, 2^30 jobs of 16 pixels; 3 such views are accepted that far
    huge = _capi.make_params(8 * 32768, 8 * 1024, 64)
    k8 = _Calls(lib, rtw, T, n=8)
    for call in (k8.accum, k8.adapt):
        assert call(huge) == -5 and b"too large" in err()
        assert call(huge, accs=None) == -1                                             # (the nulls first)
    assert k.accum(huge, 64, 1) == -2 and b"chunk range" in err()
    assert k.adapt(huge, A=_capi.Adaptive(-1.0, 0.03, 0, 0)) == -2 and b"tolerance" in err()
    # the chunk range of a progressive batch (64 spp: 64 chunks)
    for begin, count in ((-1, 1), (0, 0), (0, -1), (60, 5), (64, 1), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert k.accum(P, begin, count) == -2 and b"chunk range" in err(), (begin, count)
    # the adaptive parameters
    assert k.adapt(P, A=None) == -1
    for tol in (0.0, -0.1, float("nan"), float("inf"), -float("inf")):
        assert k.adapt(P, A=_capi.Adaptive(tol, 0.03, 0, 0)) == -2 and b"tolerance" in err(), tol
    for floor in (-1e-9, float("nan"), float("inf")):
        assert k.adapt(P, A=_capi.Adaptive(0.05, floor, 0, 0)) == -2 and b"dark_floor" in err(), floor
    for bad in (1, 3, 17, -2, -1):
        assert k.adapt(P, A=_capi.Adaptive(0.05, 0.03, bad, 0)) == -2 and b"min_chunks" in err(), bad
        assert k.adapt(P, A=_capi.Adaptive(0.05, 0.03, 0, bad)) == -2 and b"check_chunks" in err(), bad
    # precedence: bad parameters and a null -> the null is reported
    assert k.adapt(P, A=_capi.Adaptive(-1.0, 0.03, 0, 0), scene=None) == -1
    assert k.accum(P, -1, 1, accs=None) == -1


def test_python_layer_exports_and_validation(rtw):
    for name in ("ProgressiveBatchRenderer", "AdaptiveBatchRenderer", "render_adaptive_batch"):
        assert name in rtw.__all__ and hasattr(rtw, name)
    assert issubclass(rtw.AdaptiveBatchRenderer, rtw.ProgressiveBatchRenderer)
    scene = rtw.scene_2_spheres(elem_type=np.float32)
    cam = rtw.t_default_cam(elem_type=np.float32)
    with pytest.raises(TypeError):
        rtw.ProgressiveBatchRenderer(scene, [], 96, 4)
    with pytest.raises(TypeError):
        rtw.ProgressiveBatchRenderer(scene, [cam, "not a camera"], 96, 4)
    with pytest.raises(TypeError):
        rtw.AdaptiveBatchRenderer(scene, [cam, rtw.t_default_cam(elem_type=np.float64)], 96, 4)
    with pytest.raises(ValueError):
        rtw.AdaptiveBatchRenderer(scene, [cam, cam], 96, 0)
    with pytest.raises(ValueError):
        rtw.AdaptiveBatchRenderer(scene, [cam, cam], 96, 4, seeds=[1, 2, 3])
    with pytest.raises(TypeError):
        rtw.render_adaptive_batch(scene, [cam], 96, 4)             # tolerance is required
