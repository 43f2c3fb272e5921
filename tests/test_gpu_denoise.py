"""The feature-guided denoiser on the GPU (include/rtw_hip.h rtw_denoise_*) against the witness tests/denoise_ref.py.  Every comparison is
on the BITS; NaN pixels are compared as a set.  Tolerance: NONE.
Frames (width x height): 1 x 1, 5 x 3, 37 x 23 (ragged against any tile), 70 x 41 (several workgroups, pixels of one wave in two columns).  With levels = 5 the
step 16 exceeds the small frames: every tap but the centre falls outside."""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_ref as DR
import features_ref as FR
from conftest import CamObj

pytestmark = pytest.mark.gpu

FRAMES = [(1, 1), (5, 3), (37, 23), (70, 41)]          # (W, H)
SEEDS = {np.float32: 11, np.float64: 12}


@functools.lru_cache(maxsize=None)
def _frame(W, H, T):
    image, feat = DR.handmade(H, W, T, SEEDS[T])
    image.setflags(write=False)
    feat.setflags(write=False)
    return image, feat


@functools.lru_cache(maxsize=None)
def _witness(W, H, T, levels, m, demodulate, gamma):
    image, feat = _frame(W, H, T)
    out = DR.denoise(image, feat, T, levels=levels, m=m, demodulate=demodulate, gamma=gamma)
    out.setflags(write=False)
    return out


def _lib_layout(a):
    """[H, W, c] -> the library's memory: pixel (i, j) at j*H + i"""
    return np.array(a.transpose(1, 0, 2), order="C", copy=True)


def _params(levels=3, m=1, demodulate=True, gamma=1, sigma_color=0.5, sigma_depth=0.1):
    from rtw_amd import _capi
    return _capi.Denoise(levels, m, 1 if demodulate else 0, gamma, -1, 0, sigma_color, sigma_depth)


def denoise_host(image, feat, T, **kw):
    from rtw_amd import _capi
    L = _capi.lib()
    H, W = image.shape[:2]
    img, f = _lib_layout(image), _lib_layout(feat)
    out = np.full(W * H * 3, -7.0, T)
    D = _params(**kw)
    fn = L.rtw_denoise_f64 if T is np.float64 else L.rtw_denoise_f32
    _capi.check(fn(C.byref(D), W, H, img.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out.reshape(W, H, 3).transpose(1, 0, 2)


class DeviceFrame:
    """a frame's inputs as torch tensors on cuda:0, and the device entry point on them"""

    def __init__(self, image, feat, T):
        import torch
        from rtw_amd import _capi
        self.L, self.T = _capi.lib(), T
        self.H, self.W = image.shape[:2]
        self.img = torch.from_numpy(_lib_layout(image)).to("cuda:0")
        self.feat = torch.from_numpy(_lib_layout(feat)).to("cuda:0")
        self.work_bytes = int(self.L.rtw_denoise_work_bytes(self.W, self.H, np.dtype(T).itemsize))
        torch.cuda.synchronize()

    def workspace(self, poison=False):
        import torch
        w = torch.zeros(self.work_bytes // np.dtype(self.T).itemsize, dtype=self.img.dtype, device="cuda:0")
        if poison:
            w.fill_(float("nan"))
        return w

    def run(self, work=None, stream=None, **kw):
        """-> the output tensor (not synchronised when a stream is given)"""
        import torch
        from rtw_amd import _capi
        work = self.workspace() if work is None else work
        out = torch.full((self.W * self.H * 3,), -7.0, dtype=self.img.dtype, device="cuda:0")
        torch.cuda.synchronize()                                   # the fills above ran on torch's stream
        D = _params(**kw)
        fn = self.L.rtw_denoise_device_f64 if self.T is np.float64 else self.L.rtw_denoise_device_f32
        _capi.check(fn(C.byref(D), self.W, self.H, C.c_void_p(self.img.data_ptr()), C.c_void_p(self.feat.data_ptr()), C.c_void_p(out.data_ptr()),
                       C.c_void_p(work.data_ptr()), C.c_void_p(stream.cuda_stream) if stream is not None else None))
        self._keep = work
        if stream is None:
            torch.cuda.synchronize()
        return out

    def image(self, out):
        return out.cpu().numpy().reshape(self.W, self.H, 3).transpose(1, 0, 2)


def _assert_same(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: the NaN sets differ ({int(gn.sum())} vs {int(rn.sum())} values)"
    assert np.array_equal(gn.any(axis=2), gn.all(axis=2)), f"{what}: a pixel is NaN in some channels only"
    bad = (DR.bits(got) != DR.bits(ref)) & ~gn
    if bad.any():
        where = np.argwhere(bad)[:5]
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} values differ; first (i, j, c): {where.tolist()}; "
                    f"got {[got[tuple(w)] for w in where]} expected {[ref[tuple(w)] for w in where]}")


# ---- 1. every frame, precision and parameter set through both entry points -------------------------------------------------------------
@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_frames_equal_the_witness(T, W, H, entry):
    image, feat = _frame(W, H, T)
    dev = DeviceFrame(image, feat, T) if entry == "device" else None
    work = dev.workspace() if dev else None
    for levels in (1, 3, 5):
        for m in (0, 1, 7):
            for demodulate in (True, False):
                for gamma in (0, 1):
                    kw = dict(levels=levels, m=m, demodulate=demodulate, gamma=gamma)
                    ref = _witness(W, H, T, levels, m, demodulate, gamma)
                    got = dev.image(dev.run(work=work, **kw)) if dev else denoise_host(image, feat, T, **kw)
                    _assert_same(got, ref, f"{np.dtype(T).name} {W}x{H} {entry} {kw}")
    if W * H >= 12:
        assert np.isnan(ref).any() and np.isfinite(ref).any()


# ---- 2. sigma values reach the kernels; the host entry point gives the device entry point's bytes ----------------------------------------
@pytest.mark.parametrize("W,H", [(37, 23), (70, 41)])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_sigmas_and_both_entry_points(T, W, H):
    image, feat = _frame(W, H, T)
    dev = DeviceFrame(image, feat, T)
    for levels in (1, 2, 3, 5):
        a = dev.image(dev.run(levels=levels))
        _assert_same(denoise_host(image, feat, T, levels=levels), a, f"host vs device, levels={levels}")
    for sc, sz in ((0.125, 0.1), (0.5, 2.0), (3.0, 0.01)):
        ref = DR.denoise(image, feat, T, sigma_color=sc, sigma_depth=sz)
        _assert_same(dev.image(dev.run(sigma_color=sc, sigma_depth=sz)), ref, f"sigma {sc} {sz}")


# ---- 3. the workspace: poison changes nothing; two streams with a workspace each ---------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_poisoned_workspace_changes_nothing(T):
    W, H = 37, 23
    image, feat = _frame(W, H, T)
    dev = DeviceFrame(image, feat, T)
    for levels in (1, 2, 3):
        got = dev.image(dev.run(work=dev.workspace(poison=True), levels=levels))
        _assert_same(got, _witness(W, H, T, levels, 1, True, 1), f"poisoned workspace, levels={levels}")


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_two_streams_with_separate_workspaces(T):
    import torch
    W, H = 70, 41
    image, feat = _frame(W, H, T)
    dev = DeviceFrame(image, feat, T)
    single = dev.image(dev.run(levels=4))
    wa, wb = dev.workspace(), dev.workspace(poison=True)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    oa = dev.run(work=wa, stream=sa, levels=4)
    ob = dev.run(work=wb, stream=sb, levels=4)
    sa.synchronize()
    sb.synchronize()
    _assert_same(dev.image(oa), single, "stream a")
    _assert_same(dev.image(ob), single, "stream b")


# ---- 4. render + features + denoiser in one call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_render_denoised_equals_the_witness_on_the_device_renders(T):
    """frame F (32 x 18, 8 spp, 8 chunks): the witness applied to the product's own linear image and feature pass"""
    from rtw_amd import _capi
    from test_gpu_features import DeviceScene
    flat, cam, W, H = FR.frame_f(T)
    with DeviceScene(flat, T) as ds:
        img = np.ascontiguousarray(ds.image(cam, W, H, 8, 8))
        raw, _ = ds.features(cam, W, H, 8, 8, (0, 8))
        render_stats = None
    L = _capi.lib()
    S, keep = _capi.make_scene(flat, T)
    Cm = _capi.make_camera(CamObj(cam), T)
    fn = L.rtw_render_denoised_f64 if T is np.float64 else L.rtw_render_denoised_f32
    for gamma, kw in ((1, dict()), (0, dict(levels=2, m=3, demodulate=False))):
        P = _capi.make_params(width=W, height=H, spp=8, seed=1, n_chunks=8, gamma=gamma)
        D = _params(gamma=1 - gamma, **kw)                          # d->gamma is replaced by p->gamma
        out = np.full(W * H * 3, -7.0, T)
        _capi.check(fn(C.byref(S), C.byref(Cm), C.byref(P), C.byref(D), out.ctypes.data_as(C.c_void_p)))
        st = _capi.Stats()
        _capi.check(L.rtw_stats(C.byref(st)))
        ref = DR.denoise(img, np.ascontiguousarray(raw), T, gamma=gamma, **kw)
        _assert_same(out.reshape(W, H, 3).transpose(1, 0, 2), ref, f"render_denoised gamma={gamma}")
        # rtw_stats reports the render: 8 samples per pixel, more segments than samples (the feature pass has segments == samples)
        assert st.samples == W * H * 8 and st.segments > st.samples and st.n_chunks == 8 and st.kernel_ms > 0
        assert render_stats is None or (st.samples, st.segments) == render_stats
        render_stats = (st.samples, st.segments)
    del keep


# ---- 5. rtw_stats is left alone; the Python layer ----------------------------------------------------------------------------------------
def test_stats_still_report_the_previous_render(rtw):
    T = np.float32
    scene, cam = rtw.scene_2_spheres(elem_type=T), rtw.t_default_cam(elem_type=T)
    rtw.render(scene, cam, 96, 4, depth=16, seed=1, device=0)
    from rtw_amd import _capi
    L = _capi.lib()
    before = _capi.Stats()
    _capi.check(L.rtw_stats(C.byref(before)))
    image, feat = _frame(37, 23, T)
    dev = DeviceFrame(image, feat, T)
    dev.run()
    denoise_host(image, feat, T)
    after = _capi.Stats()
    _capi.check(L.rtw_stats(C.byref(after)))
    for k, _ in _capi.Stats._fields_:
        assert getattr(before, k) == getattr(after, k), k
    assert after.samples == 96 * 54 * 4


def test_python_layer(rtw):
    import torch
    T = np.float32
    W, H = 37, 23
    image, feat = _frame(W, H, T)
    ref = _witness(W, H, T, 3, 1, True, 1)
    _assert_same(rtw.denoise(image, feat), ref, "denoise")
    _assert_same(rtw.denoise(image, FR_split(feat)), ref, "denoise with the dict of render_features")
    _assert_same(rtw.denoise(image, feat, levels=5, normal_power_log2=7, demodulate=False, gamma=False),
                 _witness(W, H, T, 5, 7, False, 0), "denoise keywords")
    dev = DeviceFrame(image, feat, T)
    work, out = dev.workspace(), torch.zeros(W * H * 3, dtype=torch.float32, device="cuda:0")
    assert rtw.denoise_work_bytes(W, H, T) == dev.work_bytes
    torch.cuda.synchronize()
    rtw.denoise_into(out.data_ptr(), dev.img.data_ptr(), dev.feat.data_ptr(), work.data_ptr(), W, H, elem_type=T, work_bytes=dev.work_bytes)
    torch.cuda.synchronize()
    _assert_same(dev.image(out), ref, "denoise_into")
    # render_denoised == denoise(render(gamma=False), render_features(...)) of the same parameters
    scene, cam = rtw.scene_2_spheres(elem_type=T), rtw.t_default_cam(elem_type=T)
    got = rtw.render_denoised(scene, cam, 48, 4, seed=3)
    assert got.shape == (27, 48, 3) and got.dtype == T
    assert rtw.last_stats()["samples"] == 48 * 27 * 4
    lin = rtw.render(scene, cam, 48, 4, seed=3, gamma=False)
    f = rtw.render_features(scene, cam, 48, 4, seed=3)
    _assert_same(got, rtw.denoise(lin, f), "render_denoised vs its parts")
    _assert_same(got, DR.denoise(np.ascontiguousarray(lin), np.ascontiguousarray(f["raw"]), T), "render_denoised vs the witness")


def FR_split(raw):
    from rtw_amd.features import split
    return split(raw)
