"""First-hit feature buffers on the GPU (include/rtw_hip.h rtw_render_features_*) against the witness tests/features_ref.py -- the
definition restated from the oracle's unit calls -- and against the product's own trace kernel.  Every comparison is on the BITS (the
outputs viewed as unsigned integers); NaN pixels are compared as a set.  Tolerance: NONE."""
import ctypes as C

import numpy as np
import pytest

import features_ref as FR
from conftest import CamObj, load_golden

pytestmark = pytest.mark.gpu

SCAN_FLAGS = {"matrix": 0, "valu": 4, "cull": 1, "cull_valu": 5}      # RTW_FLAG_GROUP_CULL = 1, RTW_FLAG_SCAN_VALU = 4
PARAM_SETS = [(20, 8), (8, 8)]          # (spp, n_chunks): s = 3, N = 7 and s = 1, N = 8


def _raw(out, W, H):
    return out.reshape(W, H, 8).transpose(1, 0, 2)


def _stats(L):
    from rtw_amd import _capi
    st = _capi.Stats()
    _capi.check(L.rtw_stats(C.byref(st)))
    return st


def features_host(flat, cam, T, W, H, spp, n_chunks, chunks, seed=1, flags=0, job_pixels=0):
    """rtw_render_features_f32/_f64 -> (raw [H, W, 8], stats)"""
    from rtw_amd import _capi
    L = _capi.lib()
    S, keep = _capi.make_scene(flat, T)
    Cm = _capi.make_camera(CamObj(cam), T)
    P = _capi.make_params(width=W, height=H, spp=spp, seed=seed, n_chunks=n_chunks, flags=flags, job_pixels=job_pixels)
    out = np.full(W * H * 8, -7.0, T)
    fn = L.rtw_render_features_f64 if T is np.float64 else L.rtw_render_features_f32
    _capi.check(fn(C.byref(S), C.byref(Cm), C.byref(P), chunks[0], chunks[1], out.ctypes.data_as(C.c_void_p)))
    return _raw(out, W, H), _stats(L)


class DeviceScene:
    def __init__(self, flat, T):
        from rtw_amd import _capi
        self.L, self.T = _capi.lib(), T
        S, keep = _capi.make_scene(flat, T)
        self.handle = C.c_void_p()
        up = self.L.rtw_scene_upload_f64 if T is np.float64 else self.L.rtw_scene_upload_f32
        _capi.check(up(C.byref(S), 0, C.byref(self.handle)))

    def close(self):
        if self.handle:
            self.L.rtw_scene_free(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
        return False

    def _buffer(self, n):
        import torch
        return torch.full((n,), -7.0, dtype=torch.float64 if self.T is np.float64 else torch.float32, device="cuda:0")

    def _fetch(self, d):
        import torch
        st = _stats(self.L)                  # (waits for the call on the library's side)
        torch.cuda.synchronize()
        return d.cpu().numpy(), st

    def features(self, cam, W, H, spp, n_chunks, chunks, seed=1, flags=0, job_pixels=0):
        """rtw_render_features_device_f32/_f64 -> (raw [H, W, 8], stats)"""
        from rtw_amd import _capi
        Cm = _capi.make_camera(CamObj(cam), self.T)
        P = _capi.make_params(width=W, height=H, spp=spp, seed=seed, n_chunks=n_chunks, flags=flags, job_pixels=job_pixels)
        d = self._buffer(W * H * 8)
        fn = self.L.rtw_render_features_device_f64 if self.T is np.float64 else self.L.rtw_render_features_device_f32
        _capi.check(fn(self.handle, C.byref(Cm), C.byref(P), chunks[0], chunks[1], C.c_void_p(d.data_ptr()), None))
        out, st = self._fetch(d)
        return _raw(out, W, H), st

    def image(self, cam, W, H, spp, n_chunks, seed=1, depth=16):
        """rtw_render_device_f32/_f64 with gamma = 0 -> img [H, W, 3]"""
        from rtw_amd import _capi
        Cm = _capi.make_camera(CamObj(cam), self.T)
        P = _capi.make_params(width=W, height=H, spp=spp, max_depth=depth, seed=seed, n_chunks=n_chunks, gamma=0)
        d = self._buffer(W * H * 3)
        fn = self.L.rtw_render_device_f64 if self.T is np.float64 else self.L.rtw_render_device_f32
        _capi.check(fn(self.handle, C.byref(Cm), C.byref(P), C.c_void_p(d.data_ptr()), None))
        out, _ = self._fetch(d)
        return out.reshape(W, H, 3).transpose(1, 0, 2)


def _assert_same_bits(got, ref, what=""):
    assert got.dtype == ref.dtype and got.shape == ref.shape
    bad = FR.bits(got) != FR.bits(ref)
    if bad.any():
        where = np.argwhere(bad)[:5]
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} values differ; first (i, j, slot): {where.tolist()}; "
                    f"got {[got[tuple(w)] for w in where]} expected {[ref[tuple(w)] for w in where]}")


def _assert_stats(st, W, H, count, n_spheres, N):
    assert st.samples == st.segments == W * H * count, (st.samples, st.segments)
    assert st.sphere_tests == st.segments * n_spheres
    assert st.n_chunks == N
    assert st.kernel_ms > 0


# ---- 1. the frame F against the witness, through both entry points; 7. the counters ----------------------------------------------------
@pytest.mark.usefixtures("numerics")
@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("spp,n_chunks", PARAM_SETS)
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_frame_f_equals_the_witness(oracle, T, spp, n_chunks, entry):
    flat, cam, W, H = FR.frame_f(T)
    it = FR.items(flat, cam, W, H, spp, n_chunks, 1, T, key="F")
    ref, poisoned = FR.resolve(it, T)
    assert not poisoned.any()
    N = it["N"]
    if entry == "host":
        raw, st = features_host(flat, cam, T, W, H, spp, n_chunks, (0, N))
    else:
        with DeviceScene(flat, T) as ds:
            raw, st = ds.features(cam, W, H, spp, n_chunks, (0, N))
    assert not np.isnan(raw).any()
    _assert_same_bits(np.ascontiguousarray(raw), ref, f"{np.dtype(T).name} {spp}/{n_chunks} {entry}")
    _assert_stats(st, W, H, N, int(flat["n"]), N)       # (485 spheres in Float32, 486 in Float64)


# ---- 2. scan modes and job sizes: identical bytes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_modes_and_job_sizes_give_identical_bytes(oracle, T):
    flat, cam, W, H = FR.frame_f(T)
    ref, _ = FR.resolve(FR.items(flat, cam, W, H, 20, 8, 1, T, key="F"), T)
    with DeviceScene(flat, T) as ds:
        for scan, flags in SCAN_FLAGS.items():
            for jp in (0, 1, 16):
                raw, _ = ds.features(cam, W, H, 20, 8, (0, 7), flags=flags, job_pixels=jp)
                _assert_same_bits(np.ascontiguousarray(raw), ref, f"{scan} job_pixels={jp}")
    raw, _ = features_host(flat, cam, T, W, H, 20, 8, (0, 7), flags=SCAN_FLAGS["cull_valu"], job_pixels=4)
    _assert_same_bits(np.ascontiguousarray(raw), ref, "host cull_valu job_pixels=4")


# ---- 3. chunk ranges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.usefixtures("numerics")
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_chunk_ranges_equal_the_witness(oracle, T):
    """(0, 1): the centred sample alone, no jitter draw; (2, 3): an inner range; (6, 1): the last, short chunk"""
    flat, cam, W, H = FR.frame_f(T)
    it = FR.items(flat, cam, W, H, 20, 8, 1, T, key="F")
    with DeviceScene(flat, T) as ds:
        for chunks in ((0, 1), (2, 3), (6, 1)):
            ref, poisoned = FR.resolve(it, T, chunks)
            assert not poisoned.any()
            raw, st = ds.features(cam, W, H, 20, 8, chunks)
            _assert_same_bits(np.ascontiguousarray(raw), ref, f"chunks {chunks}")
            _assert_stats(st, W, H, chunks[1], int(flat["n"]), 7)
            for scan in ("valu", "cull"):
                raw2, _ = ds.features(cam, W, H, 20, 8, chunks, flags=SCAN_FLAGS[scan])
                _assert_same_bits(np.ascontiguousarray(raw2), ref, f"chunks {chunks} {scan}")


# ---- 4. small and awkward scenes --------------------------------------------------------------------------------------------------------
@pytest.mark.usefixtures("numerics")
@pytest.mark.parametrize("scan", ["matrix", "valu"])
@pytest.mark.parametrize("name", ["cfg1_2spheres_96x54_16spp_d4_f32",      # fewer than 32 spheres: one block, the caller's order kept
                                  "diel_bubble_96x54_8spp_d16_f32",        # a negative radius flips the outward normal
                                  "metal4_96x54_8spp_d16_f32"])
def test_small_scenes_equal_the_witness(oracle, name, scan):
    """24 x 13: ragged in both directions (3 x 2 tiles, the last row of tiles 5 pixels high); spp = 7 in 3 chunks: s = 3, the last chunk short"""
    g = load_golden(name)
    T = g["image"].dtype.type
    W, H, spp, n_chunks = 24, 13, 7, 3
    it = FR.items(g["flat"], g["cam"], W, H, spp, n_chunks, g["seed"], T, key=name)
    assert (it["N"], it["s"]) == (3, 3)
    ref, poisoned = FR.resolve(it, T)
    assert not poisoned.any() and (ref[..., 7] > 0).any()
    raw, st = features_host(g["flat"], g["cam"], T, W, H, spp, n_chunks, (0, 3), seed=g["seed"], flags=SCAN_FLAGS[scan])
    _assert_same_bits(np.ascontiguousarray(raw), ref, f"{name} {scan}")
    _assert_stats(st, W, H, 3, g["flat"]["n"], 3)
    if name.startswith("diel_bubble"):
        assert 2 in set(np.unique(it["kind"]))                     # the dielectric spheres are seen


# ---- 5. against the product's own trace kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_uncovered_pixels_equal_the_trace_kernels_image(T):
    """spp = 8 in 8 chunks (s = 1): the feature samples are ALL the primary rays of the image; where none of them hits, the linear image
    (gamma = 0) is the mean of their sky colours -- the albedo slots, through the same exact sums"""
    flat, cam, W, H = FR.frame_f(T)
    with DeviceScene(flat, T) as ds:
        raw, _ = ds.features(cam, W, H, 8, 8, (0, 8))
        img = ds.image(cam, W, H, 8, 8)
    empty = raw[..., 7] == 0
    assert int(empty.sum()) >= 40
    _assert_same_bits(np.ascontiguousarray(raw[..., 0:3][empty]), np.ascontiguousarray(img[empty]), "albedo of uncovered pixels vs the image")
    assert not raw[..., 3:7][empty].any()


# ---- 6. poison --------------------------------------------------------------------------------------------------------------------------
def test_a_depth_beyond_2_31_poisons_the_pixel(oracle):
    """one sphere of radius 1e9 at z = -1e10 seen from the origin: t ~ 9e9 > 2^31 where it is hit"""
    T = np.float32
    flat = dict(n=1, cx=np.array([0], T), cy=np.array([0], T), cz=np.array([-1e10], T), r=np.array([1e9], T), kind=np.array([0], np.int32),
                ar=np.array([0.5], T), ag=np.array([0.25], T), ab=np.array([0.125], T), param=np.array([0], T))
    cam = oracle.default_camera([0, 0, 0], [0, 0, -1], [0, 1, 0], 90, 16 / 9, 0.0, 1, T)
    W, H, spp = 16, 9, 4
    it = FR.items(flat, cam, W, H, spp, 0, 1, T)
    ref, poisoned = FR.resolve(it, T)
    assert poisoned.any() and not poisoned.all()
    assert it["values"][..., 6].max() > 2.0 ** 31
    for scan in ("matrix", "valu"):
        raw, _ = features_host(flat, cam, T, W, H, spp, 0, (0, 4), flags=SCAN_FLAGS[scan])
        nan = np.isnan(raw)
        assert np.array_equal(nan.any(axis=2), poisoned), scan               # the same pixels ...
        assert np.array_equal(nan.all(axis=2), poisoned), scan               # ... NaN in all 8 slots
        assert np.isfinite(raw[~poisoned]).all()
        _assert_same_bits(np.ascontiguousarray(raw[~poisoned]), np.ascontiguousarray(ref[~poisoned]), f"unpoisoned pixels {scan}")


# ---- the refusal that needs a real handle; the Python layer ------------------------------------------------------------------------------
def test_a_scene_of_the_other_precision_is_refused(rtw):
    import torch
    from rtw_amd import _capi
    flat, cam, W, H = FR.frame_f(np.float32)
    with DeviceScene(flat, np.float32) as ds:
        Cm = _capi.make_camera(CamObj(cam), np.float64)
        P = _capi.make_params(width=W, height=H, spp=8)
        d = torch.zeros(W * H * 8, dtype=torch.float64, device="cuda:0")
        assert ds.L.rtw_render_features_device_f64(ds.handle, C.byref(Cm), C.byref(P), 0, 8, C.c_void_p(d.data_ptr()), None) == -4
        assert b"precision" in ds.L.rtw_last_error()


def test_python_layer(rtw):
    import torch
    T = np.float32
    scene, cam = rtw.scene_2_spheres(elem_type=T), rtw.t_default_cam(elem_type=T)
    f = rtw.render_features(scene, cam, 24, 7, n_chunks=3)
    assert f["raw"].shape == (13, 24, 8) and f["albedo"].shape == (13, 24, 3) and f["normal"].shape == (13, 24, 3)
    assert f["depth"].shape == f["coverage"].shape == (13, 24) and f["raw"].dtype == T
    assert rtw.last_stats()["segments"] == 24 * 13 * 3
    part = rtw.render_features(scene, cam, 24, 7, n_chunks=3, chunks=(1, 2), flags=SCAN_FLAGS["valu"])
    dr = rtw.DeviceRenderer(scene, cam, device=0)
    try:
        d = torch.zeros(24 * 13 * 8, dtype=torch.float32, device="cuda:0")
        assert dr.features_into(d.data_ptr(), 24, 7, n_chunks=3, chunks=(1, 2), n_elems=d.numel()) == 13
        st = dr.stats()
        torch.cuda.synchronize()
        assert st["segments"] == 24 * 13 * 2
        _assert_same_bits(np.ascontiguousarray(_raw(d.cpu().numpy(), 24, 13)), np.ascontiguousarray(part["raw"]), "features_into vs render_features")
        with pytest.raises(ValueError):
            dr.features_into(d.data_ptr(), 24, 7, n_elems=10)
    finally:
        dr.close()
