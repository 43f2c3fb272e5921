"""Present stage (include/rtw_hip.h ``rtw_present_*``): display-ready 8-bit frames from the device.  Every other pipeline of the library ends in
float elements in the column-major layout of ``Matrix{RGB{T}}``; this one clips, rounds, packs and transposes them in HBM into row-major
``uint8 [H, W, C]`` -- what a window, a PNG or a video encoder takes -- so the D2H moves 3 or 4 bytes per pixel and the host converts nothing.
The definition is in the header; tests/present_ref.py restates it on the CPU and the device agrees on the bytes.  With the defaults the
result is ``imageio.to_u8`` of the same frame on the bits.  All compute happens in librtw_hip.so; there is no CPU fallback.

Defaults: ``channels=3, dither=False, bgr=False, sqrt=False, exposure=1.0, nan_rgb=(0, 0, 0)``.
"""
import ctypes as C

import numpy as np

from . import _capi
from .denoise import make_denoise
from .render import _batch_cameras, _frame_height, _record_stats
from .structs import Camera, flatten_scene


def make_present(channels=3, dither=False, bgr=False, sqrt=False, exposure=1.0, nan_rgb=(0, 0, 0), device=-1):
    """-> the ``rtw_present_t`` of these keywords"""
    flags = (_capi.PRESENT_DITHER if dither else 0) | (_capi.PRESENT_BGR if bgr else 0) | (_capi.PRESENT_SQRT if sqrt else 0)
    if int(channels) not in (3, 4):
        raise ValueError("channels must be 3 or 4")
    nan = [int(v) for v in nan_rgb]
    if len(nan) != 3 or any(v < 0 or v > 255 for v in nan):
        raise ValueError("nan_rgb must be three bytes")
    return _capi.Present(int(channels), flags, int(device), (C.c_uint8 * 3)(*nan), 0, float(exposure), (C.c_int32 * 2)(0, 0))


def present_bytes(image_width, image_height, channels=3, n_views=0):
    """bytes of the output of ``n_views`` frames (0: one frame)"""
    n = _capi.lib().rtw_present_bytes(int(image_width), int(image_height), int(channels), int(n_views))
    if n < 0:
        _capi.check(int(n))
    return int(n)


def present(image, **kw):
    """``image`` [H, W, 3], a host array of float32 or float64 -> ``uint8 [H, W, C]``, C-contiguous, as the library wrote it
    (rtw_present_*).  Keywords: ``make_present``.  Blocking; ``last_stats()`` is left as it was."""
    image = np.asarray(image)
    T = image.dtype
    if T not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("image must be float32 or float64")
    if image.ndim != 3 or image.shape[-1] != 3:
        raise ValueError(f"expected image [H, W, 3], got {image.shape}")
    if 0 in image.shape:
        raise ValueError("empty image")
    H, W = image.shape[:2]
    P = make_present(**kw)
    img = np.ascontiguousarray(np.swapaxes(image, 0, 1))             # the library's layout: pixel (i, j) at j*H + i
    out = np.empty((H, W, P.channels), dtype=np.uint8)
    fn = getattr(_capi.lib(), "rtw_present_" + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(C.byref(P), W, H, img.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def present_into(d_out_ptr, d_image_ptr, image_width, image_height, *, elem_type=np.float32, stream=0, **kw):
    """The device-resident form (rtw_present_device_*): enqueue ONE launch on ``stream``.  Both are DEVICE pointers (a torch tensor's
    ``data_ptr()``): the image holds H*W*3 elements in the render's layout, the result ``present_bytes(...)`` bytes, 4-byte aligned; they
    may not overlap.  Keywords: ``make_present``."""
    P = make_present(**kw)
    fn = getattr(_capi.lib(), "rtw_present_device_" + ("f64" if _capi.is_f64(elem_type) else "f32"))
    _capi.check(fn(C.byref(P), int(image_width), int(image_height), C.c_void_p(int(d_image_ptr)), C.c_void_p(int(d_out_ptr)), C.c_void_p(int(stream))))


def present_batch_into(d_out_ptr, d_images_ptr, image_width, image_height, n_views, *, elem_type=np.float32, stream=0, **kw):
    """The device-resident batched form (rtw_present_batch_device_*): ``present_into`` for ``n_views`` frames one behind the other in both
    buffers, in the same ONE launch.  View ``v`` is byte for byte ``present_into`` on frame ``v``."""
    if int(n_views) < 1:
        raise ValueError("n_views must be >= 1")
    P = make_present(**kw)
    fn = getattr(_capi.lib(), "rtw_present_batch_device_" + ("f64" if _capi.is_f64(elem_type) else "f32"))
    _capi.check(fn(C.byref(P), int(image_width), int(image_height), int(n_views), C.c_void_p(int(d_images_ptr)), C.c_void_p(int(d_out_ptr)),
                   C.c_void_p(int(stream))))


def _render_presented(scene, T, Cm, n, sd, image_width, n_samples, depth, seed, n_chunks, device, gamma, group_cull, scan_valu, numerics, denoise, pk):
    """Both one-call forms behind their camera checks -> uint8 [max(n, 1), H, W, C].  n == 0: rtw_render_presented_* through the one camera
    ``Cm``; n >= 1: rtw_render_presented_batch_* through the n cameras ``Cm`` with the seeds ``sd``.  ``pk``: ``make_present``'s keywords."""
    height = _frame_height(image_width, n_samples)
    L = _capi.lib()
    flat = scene if isinstance(scene, dict) else flatten_scene(scene, T)
    S, keep = _capi.make_scene(flat, T)
    P = _capi.make_params(image_width, height, n_samples, depth, seed, n_chunks, 0, 1, device, 1 if gamma else 0,
                          (_capi.FLAG_GROUP_CULL if group_cull else 0) | (_capi.FLAG_SCAN_VALU if scan_valu else 0), numerics=numerics)
    if denoise is None or denoise is False:
        D = None
    else:
        D = C.byref(make_denoise(**({} if denoise is True else dict(denoise))))
    Pr = make_present(**pk)
    out = np.empty((max(n, 1), height, int(image_width), Pr.channels), dtype=np.uint8)
    sfx = "f64" if _capi.is_f64(T) else "f32"
    if n:
        rc = getattr(L, "rtw_render_presented_batch_" + sfx)(C.byref(S), Cm, n, sd, C.byref(P), D, C.byref(Pr), out.ctypes.data_as(C.c_void_p))
    else:
        rc = getattr(L, "rtw_render_presented_" + sfx)(C.byref(S), C.byref(Cm), C.byref(P), D, C.byref(Pr), out.ctypes.data_as(C.c_void_p))
    _capi.check(rc)
    del keep
    _record_stats(L)
    return out


def render_presented(scene, cam, image_width=400, n_samples=1, *, denoise=None, depth=16, seed=1, n_chunks=0, device=-1, gamma=True,
                     group_cull=False, scan_valu=False, numerics=None, **present_kw):
    """``render`` (or, with ``denoise``, ``render_denoised``) + ``present`` in one call on the device (rtw_render_presented_*): the float
    frame stays in HBM, the bytes come back once.  ``denoise``: None (no filter), True (``make_denoise``'s defaults) or a dict of its
    keywords; the filter's gamma and device are the render's.  Further keywords: ``make_present``.  Returns ``uint8 [H, W, C]``;
    ``last_stats()`` reports the render."""
    if not isinstance(cam, Camera):
        raise TypeError("cam must be a Camera")
    T = cam.elem_type
    return _render_presented(scene, T, _capi.make_camera(cam, T), 0, None, image_width, n_samples, depth, seed, n_chunks, device, gamma, group_cull, scan_valu,
                             numerics, denoise, present_kw)[0]


def render_presented_batch(scene, cams, image_width=400, n_samples=1, *, seeds=None, denoise=None, depth=16, seed=1, n_chunks=0, device=-1,
                           gamma=True, group_cull=False, scan_valu=False, numerics=None, **present_kw):
    """``render_batch`` (or, with ``denoise``, ``render_denoised_batch``) + ``present_batch_into`` in one call on the device
    (rtw_render_presented_batch_*).  Returns ``uint8 [N, H, W, C]``; view ``v`` is byte for byte
    ``render_presented(scene, cams[v], ..., seed=seeds[v])``.  ``last_stats()`` reports the render."""
    cams, T = _batch_cameras(cams)
    sd = _capi.make_seeds(seed if seeds is None else seeds, len(cams))
    return _render_presented(scene, T, _capi.make_cameras(cams, T), len(cams), sd, image_width, n_samples, depth, seed, n_chunks, device, gamma, group_cull,
                             scan_valu, numerics, denoise, present_kw)
