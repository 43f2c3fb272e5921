"""Motion blur (include/rtw_hip.h ``rtw_velocity_blur_*``): a velocity-guided gather on the motion plane.  The 1-spp animation path renders
every moving sphere sharp; this stage blurs a finished LINEAR frame along the motion the plane of ``first_hit_motion`` records -- a
deterministic form of McGuire et al. 2012: the per-pixel half-extent, its maximum per 16 x 16 tile and over the tile's neighbourhood, then
``taps`` taps along that dominant velocity under soft depth and velocity-aware weights.  It sits between the last linear stage (the step or
the filter) and the present stage, reads no temporal state and writes none: never feed its output back into the history.  The definition
is in the header; tests/motion_blur_ref.py restates it on the CPU, twice, and the device agrees on the bits.  All compute happens in
librtw_hip.so; there is no CPU fallback.

Defaults: ``taps=15, shutter=1.0, depth_extent=0.5, gamma=True``; what they buy on the CPU witness: DESIGN.md section 7.24.
"""
import ctypes as C

import numpy as np

from . import _capi
from .structs import Camera

_BLUR_KEYS = ("taps", "shutter", "depth_extent")


def make_motion_blur(taps=15, shutter=1.0, depth_extent=0.5, gamma=True, device=-1):
    """-> the ``rtw_velocity_blur_t`` of these keywords: ``taps`` odd in 3..31, ``shutter`` in (0, 1] (the fraction of the frame interval the
    shutter is open, centred on the frame's time), ``depth_extent`` > 0 in world units (the softness of the depth compare)"""
    return _capi.VelocityBlur(int(taps), 0, 1 if gamma else 0, int(device), (C.c_int32 * 2)(0, 0), float(shutter), float(depth_extent))


def motion_blur_work_bytes(image_width, image_height, elem_type=np.float32):
    """bytes of the caller-owned workspace: the blur plane (4 elements per pixel: h.x, h.y, depth, length), then the tile plane and the
    neighbour plane (4 elements per 16 x 16 tile each)"""
    n = _capi.lib().rtw_velocity_blur_work_bytes(int(image_width), int(image_height), np.dtype(elem_type).itemsize)
    if n < 0:
        _capi.check(int(n))
    return int(n)


def _camera_arg(cam, T, what):
    if not isinstance(cam, Camera):
        raise TypeError(f"{what} must be a Camera")
    if np.dtype(cam.elem_type) != np.dtype(T):
        raise TypeError(f"{what} has element type {np.dtype(cam.elem_type).name}, the frame {np.dtype(T).name}")
    return _capi.make_camera(cam, T)


def motion_blur(image, features, motion, cam, cam_prev, **params):
    """The stage on host arrays (rtw_velocity_blur_*): ``image`` [H, W, 3] (linear), ``features`` [H, W, 8] -- or the dict ``render_features``
    returns -- and ``motion`` [H, W, 4] (``first_hit_motion``) of the frame seen through ``cam``; ``cam_prev``: the previous frame's camera.
    -> the blurred image [H, W, 3]; a pixel that is not valid is NaN.  Keywords: ``make_motion_blur``.  Blocking."""
    if isinstance(features, dict):
        features = features["raw"]
    image, features, motion = np.asarray(image), np.asarray(features), np.asarray(motion)
    T = image.dtype
    if T not in (np.dtype(np.float32), np.dtype(np.float64)) or features.dtype != T or motion.dtype != T:
        raise TypeError("image, features and motion must all be float32 or all float64")
    if image.ndim != 3 or image.shape[-1] != 3 or features.shape != image.shape[:-1] + (8,) or motion.shape != image.shape[:-1] + (4,):
        raise ValueError(f"expected image [H, W, 3], features [H, W, 8] and motion [H, W, 4], got {image.shape}, {features.shape} and {motion.shape}")
    if 0 in image.shape:
        raise ValueError("empty image")
    H, W = image.shape[:2]
    Cm, Cp = _camera_arg(cam, T.type, "cam"), _camera_arg(cam_prev, T.type, "cam_prev")
    img, feat, mv = (np.ascontiguousarray(np.swapaxes(a, 0, 1)) for a in (image, features, motion))      # the library's layout: pixel (i, j) at j*H + i
    out = np.empty((W, H, 3), dtype=T)
    fn = getattr(_capi.lib(), "rtw_velocity_blur_" + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(C.byref(make_motion_blur(**params)), C.byref(Cm), C.byref(Cp), W, H, *(a.ctypes.data_as(C.c_void_p) for a in (img, feat, mv, out))))
    return np.swapaxes(out, 0, 1)


def motion_blur_into(d_out_ptr, d_work_ptr, d_image_ptr, d_features_ptr, d_motion_ptr, cam, cam_prev, image_width, image_height, *, elem_type=np.float32, stream=0,
                     **params):
    """The device-resident stage (rtw_velocity_blur_device_*): three launches on ``stream``.  DEVICE pointers in the library's layout (pixel
    (i, j) at slot ``j*H + i``): the linear image, the features, the motion plane; ``d_work_ptr``: ``motion_blur_work_bytes`` bytes, 16-byte
    aligned, which afterwards hold the blur plane, the tile plane and the neighbour plane; ``d_out_ptr`` aliases nothing.  Keywords:
    ``make_motion_blur``."""
    T = np.dtype(elem_type).type
    Cm, Cp = _camera_arg(cam, T, "cam"), _camera_arg(cam_prev, T, "cam_prev")
    fn = getattr(_capi.lib(), "rtw_velocity_blur_device_" + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(C.byref(make_motion_blur(**params)), C.byref(Cm), C.byref(Cp), int(image_width), int(image_height),
                   *(C.c_void_p(int(q)) for q in (d_image_ptr, d_features_ptr, d_motion_ptr, d_work_ptr, d_out_ptr)), C.c_void_p(int(stream))))
