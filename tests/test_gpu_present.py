"""The present stage on the GPU (include/rtw_hip.h rtw_present_*) against the witness tests/present_ref.py.  Every comparison is on the BYTES.
Tolerance: NONE.
Frames (width x height): 1 x 1; 96 x 54 (3 W a multiple of 4: the aligned-row path of C = 3, partial tiles both ways); 67 x 35 (3 W = 201: the
unaligned-row path of C = 3, rows starting at every byte of a dword); 5 x 130 and 130 x 5 (less than a tile one way, more than two the other);
64 x 64 and 65 x 65 (on and just past the tile).  The output always lies between two 64-byte guards in a buffer pre-filled with a sentinel."""
import ctypes as C
import functools

import numpy as np
import pytest

import present_ref as PR

pytestmark = pytest.mark.gpu

FRAMES = [(1, 1), (96, 54), (67, 35), (5, 130), (130, 5), (64, 64), (65, 65)]          # (W, H)
GUARD, SENTINEL = 64, 0xA5
NAN_RGB = (9, 8, 7)


def _lib_layout(a):
    """[..., H, W, 3] -> the library's memory: pixel (i, j) of a view at j*H + i"""
    return np.array(np.swapaxes(a, -3, -2), order="C", copy=True)


@functools.lru_cache(maxsize=None)
def _random_frame(W, H, T, seed=0):
    """values around [0, 1] with NaNs sprinkled in, single channels and whole pixels"""
    rng = np.random.default_rng(1000 * W + H + seed)
    img = rng.uniform(-0.2, 1.2, (H, W, 3)).astype(T)
    img[rng.uniform(size=(H, W, 3)) < 0.03] = np.nan
    img[rng.uniform(size=(H, W)) < 0.02] = np.nan
    img.setflags(write=False)
    return img


def _params(channels=3, flags=0, exposure=1.0, nan_rgb=NAN_RGB):
    from rtw_amd import _capi
    return _capi.Present(channels, flags, -1, (C.c_uint8 * 3)(*nan_rgb), 0, exposure, (C.c_int32 * 2)(0, 0))


class DeviceFrames:
    """one frame [H, W, 3] or a batch [N, H, W, 3] as a torch tensor on cuda:0, and the device entry points on it"""

    def __init__(self, images, T):
        import torch
        from rtw_amd import _capi
        self.L, self.T = _capi.lib(), T
        self.N = images.shape[0] if images.ndim == 4 else 0
        self.H, self.W = images.shape[-3:-1]
        self.img = torch.from_numpy(_lib_layout(images)).to("cuda:0")
        torch.cuda.synchronize()

    def run(self, stream=None, **kw):
        """-> uint8 [H, W, C] (or [N, H, W, C]); the guards around the output are checked"""
        import torch
        from rtw_amd import _capi
        P = _params(**kw)
        frames = max(self.N, 1)
        n = frames * self.H * self.W * P.channels
        buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        if stream is None:
            torch.cuda.synchronize()                               # the fill above ran on torch's stream (a stream given: it is torch's current one)
        sfx = "f64" if self.T is np.float64 else "f32"
        st = C.c_void_p(stream.cuda_stream) if stream is not None else None
        ptrs = (C.c_void_p(self.img.data_ptr()), C.c_void_p(buf.data_ptr() + GUARD), st)
        if self.N:
            _capi.check(getattr(self.L, "rtw_present_batch_device_" + sfx)(C.byref(P), self.W, self.H, self.N, *ptrs))
        else:
            _capi.check(getattr(self.L, "rtw_present_device_" + sfx)(C.byref(P), self.W, self.H, *ptrs))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + n:] == SENTINEL).all(), "a guard byte was written"
        shape = (self.H, self.W, P.channels)
        return got[GUARD:GUARD + n].reshape(((self.N,) if self.N else ()) + shape)


def _assert_same(got, ref, what):
    assert got.dtype == np.uint8 and got.shape == ref.shape, what
    bad = got != ref
    if bad.any():
        where = np.argwhere(bad)[:5]
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} bytes differ; first {where.tolist()}; got {[int(got[tuple(w)]) for w in where]} "
                    f"expected {[int(ref[tuple(w)]) for w in where]}")


# ---- 1. the hand-made tables: special values and rounding ties, every flag combination and exposure ---------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_tables_equal_the_witness(T):
    ties, _ = PR.tie_table()
    frames = [PR.as_frame(PR.special_values(T), T, 5), PR.as_frame(ties, T, 17), PR.as_frame(ties, T, 20)]
    n_ties = 0
    for img in frames:
        dev = DeviceFrames(img, T)
        for channels in (3, 4):
            for flags in range(8):
                for exposure in (1.0, 0.5, 3.0):
                    kw = dict(channels=channels, flags=flags, exposure=exposure)
                    ref = PR.present(img, nan_rgb=NAN_RGB, **kw)
                    _assert_same(dev.run(**kw), ref, f"{np.dtype(T).name} table {img.shape} {kw}")
        with np.errstate(all="ignore"):                                    # (the special values: NaN, inf, the largest finite)
            y = img.astype(np.float64) * 255.0
            n_ties += int((y - np.floor(y) == 0.5).sum())
    assert n_ties >= (2 * 128 if T is np.float64 else 1)                 # the ties-to-even branch was reached (binary32 holds 0.5 alone)


def test_defaults_are_to_u8_of_the_frame(rtw):
    for T in (np.float32, np.float64):
        img = _random_frame(96, 54, T)
        got = DeviceFrames(img, T).run(nan_rgb=(0, 0, 0))
        _assert_same(got, rtw.imageio.to_u8(img), f"{np.dtype(T).name} against to_u8")


# ---- 2. the shapes at which a path can go wrong ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_shapes_equal_the_witness(T, W, H):
    img = _random_frame(W, H, T)
    dev = DeviceFrames(img, T)
    for channels in (3, 4):
        for flags in (0, PR.DITHER, PR.BGR | PR.SQRT, 7):
            kw = dict(channels=channels, flags=flags, exposure=1.0 if flags != 7 else 0.5)
            _assert_same(dev.run(**kw), PR.present(img, nan_rgb=NAN_RGB, **kw), f"{np.dtype(T).name} {W}x{H} {kw}")
    if W * H > 100:
        nan = np.isnan(img)
        assert nan.any() and (nan.any(axis=2) & ~nan.all(axis=2)).any()       # NaN pixels and pixels with a NaN channel


# ---- 3. a batch is its single calls ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_batch_equals_its_single_calls(T):
    W, H = 67, 35                                                             # (a frame of 3 W H = 7035 bytes: views 1 and 2 start off a dword)
    views = np.stack([_random_frame(W, H, T, seed=s) for s in (1, 2, 3)])
    batch = DeviceFrames(views, T)
    for channels in (3, 4):
        for flags in (0, 7):
            kw = dict(channels=channels, flags=flags)
            got = batch.run(**kw)
            assert got.shape == (3, H, W, channels)
            for v in range(3):
                _assert_same(got[v], DeviceFrames(views[v], T).run(**kw), f"{np.dtype(T).name} view {v} {kw}")
                _assert_same(got[v], PR.present(views[v], nan_rgb=NAN_RGB, **kw), f"{np.dtype(T).name} view {v} {kw} against the witness")


# ---- 4. a stream of the caller's ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_device_call_runs_behind_a_fill_on_the_callers_stream(T):
    import torch
    W, H = 96, 54
    dev = DeviceFrames(np.zeros((H, W, 3), T), T)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev.img.fill_(0.5)
        got = dev.run(stream=s)
    assert (got == 128).all()                                                 # 0.5 * 255 = 127.5: the tie, to even


# ---- 5. render and present in one call ------------------------------------------------------------------------------------------------------
def _cams(rtw, T):
    return [rtw.t_default_cam(elem_type=T), rtw.default_camera((0.5, 0.3, 0.2), (0, 0, -1), (0, 1, 0), 60, 16 / 9, 0.0, 1.0, elem_type=T),
            rtw.t_cam2(elem_type=T)]


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_render_presented_equals_the_float_calls(rtw, T):
    scene = rtw.scene_2_spheres(elem_type=T)
    cams = _cams(rtw, T)
    kw = dict(depth=16, seed=3, gamma=True)
    ref = rtw.render(scene, cams[0], 96, 16, **kw)
    samples = rtw.last_stats()["samples"]
    got = rtw.render_presented(scene, cams[0], 96, 16, **kw)
    assert got.shape == (54, 96, 3) and got.flags.c_contiguous and rtw.last_stats()["samples"] == samples == 96 * 54 * 16
    _assert_same(got, rtw.imageio.to_u8(ref), f"{np.dtype(T).name} render_presented")
    got4 = rtw.render_presented(scene, cams[0], 96, 16, channels=4, bgr=True, **kw)
    _assert_same(got4, PR.present(np.asarray(ref), channels=4, flags=PR.BGR), f"{np.dtype(T).name} render_presented, BGRA")
    # with the filter
    ref = rtw.render_denoised(scene, cams[0], 96, 16, **kw)
    samples = rtw.last_stats()["samples"]
    got = rtw.render_presented(scene, cams[0], 96, 16, denoise=True, **kw)
    assert rtw.last_stats()["samples"] == samples
    _assert_same(got, rtw.imageio.to_u8(ref), f"{np.dtype(T).name} render_presented with the filter")
    # the batch: three cameras, three seeds
    for denoise in (None, dict(levels=2)):
        batch = rtw.render_presented_batch(scene, cams, 96, 16, seeds=[3, 4, 5], denoise=denoise, depth=16, gamma=True)
        assert batch.shape == (3, 54, 96, 3) and rtw.last_stats()["samples"] == 3 * samples
        for v in range(3):
            single = rtw.render_presented(scene, cams[v], 96, 16, denoise=denoise, depth=16, seed=3 + v, gamma=True)
            _assert_same(batch[v], single, f"{np.dtype(T).name} view {v} of the batch, denoise={denoise}")


# ---- 6. the host form -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_host_form_equals_the_device_form(rtw, T):
    for W, H in ((67, 35), (96, 54)):
        img = _random_frame(W, H, T)
        dev = DeviceFrames(img, T)
        for channels in (3, 4):
            got = rtw.present(img, channels=channels, dither=True, exposure=0.5, nan_rgb=NAN_RGB)
            assert got.shape == (H, W, channels) and got.flags.c_contiguous and got.flags.owndata
            _assert_same(got, dev.run(channels=channels, flags=PR.DITHER, exposure=0.5), f"{np.dtype(T).name} {W}x{H} C={channels} host vs device")
