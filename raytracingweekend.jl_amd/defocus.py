"""Depth of field (include/rtw_hip.h ``rtw_defocus_*``): a gather on a finished pinhole frame.  Every stage behind the trace kernel takes its
guides from the centre ray of a pinhole camera, so a frame rendered through a real aperture is noisy exactly where the guides no longer
describe it.  This stage applies the lens afterwards: the circle of confusion of every pixel from the depth plane of the feature buffer,
its maximum per 16 x 16 tile, then a gather over up to 17 x 17 taps in which a tap behind the pixel never spreads further than the pixel's
own circle.  It sits behind the last linear stage (the render, the filter or the temporal step) and in front of the present stage.  The
definition is in the header; tests/defocus_ref.py restates it on the CPU, twice, and the device agrees on the bits.  All compute happens
in librtw_hip.so; there is no CPU fallback.

Defaults: ``max_radius=8, focus_dist=0`` (the camera's own focus plane), ``gamma=True``; what they buy on the CPU witness: DESIGN.md section 7.25.
"""
import ctypes as C

import numpy as np

from . import _capi
from .denoise import make_denoise
from .render import _batch_cameras, _frame_height, _record_stats
from .structs import Camera, flatten_scene

_DEFOCUS_KEYS = ("lens_radius", "focus_dist", "max_radius")
_DENOISE_KEYS = ("levels", "normal_power_log2", "sigma_color", "sigma_depth", "demodulate")


def make_defocus(lens_radius, focus_dist=0.0, max_radius=8, gamma=True, device=-1):
    """-> the ``rtw_defocus_t`` of these keywords: ``lens_radius`` >= 0 in world units (half the aperture), ``focus_dist`` > 0 to override the
    camera's own focus plane (0: keep it), ``max_radius`` in 1..8: where the circle of confusion is clamped, in pixels.  The radius of a point
    at infinity, ``K = lens_radius * W / |horizontal|`` pixels, is measured on the camera's OWN focus plane and does not move with the override:
    for the lens of a camera refocused at f' pass ``lens_radius * f / f'``"""
    return _capi.Defocus(int(max_radius), 0, 1 if gamma else 0, int(device), (C.c_int32 * 2)(0, 0), float(lens_radius), float(focus_dist))


def defocus_work_bytes(image_width, image_height, elem_type=np.float32):
    """bytes of the caller-owned workspace: the CoC plane (4 elements per pixel: radius, depth, weight, 0), then the tile plane (one element
    per 16 x 16 tile, rounded up to a multiple of four)"""
    n = _capi.lib().rtw_defocus_work_bytes(int(image_width), int(image_height), np.dtype(elem_type).itemsize)
    if n < 0:
        _capi.check(int(n))
    return int(n)


def _camera_arg(cam, T, what):
    if not isinstance(cam, Camera):
        raise TypeError(f"{what} must be a Camera")
    if np.dtype(cam.elem_type) != np.dtype(T):
        raise TypeError(f"{what} has element type {np.dtype(cam.elem_type).name}, the frame {np.dtype(T).name}")
    return _capi.make_camera(cam, T)


# ---- what the lens stages share (this module, wide_aperture.py): the array checks, the device-resident call, the one-call body --------

def _entry(name, T):
    return getattr(_capi.lib(), name + ("f64" if _capi.is_f64(T) else "f32"))


def _host_arrays(image, features, batch=False):
    """the checks of a lens stage's host arrays -- ``image`` [H, W, 3] and ``features`` [H, W, 8] (or the dict a feature pass returns); ``batch``:
    [N, H, W, 3] and [N, H, W, 8] -- and their transposition -> (dtype, image, features) in the library's layout: pixel (i, j) (of view v) at
    (v*W*H +) j*H + i"""
    if isinstance(features, dict):
        features = features["raw"]
    image, features = np.asarray(image), np.asarray(features)
    T = image.dtype
    name, lead = ("images", "N, ") if batch else ("image", "")
    if T not in (np.dtype(np.float32), np.dtype(np.float64)) or features.dtype != T:
        raise TypeError(f"{name} and features must both be float32 or both float64")
    if image.ndim != (4 if batch else 3) or image.shape[-1] != 3 or features.shape != image.shape[:-1] + (8,):
        raise ValueError(f"expected {name} [{lead}H, W, 3] and features [{lead}H, W, 8], got {image.shape} and {features.shape}")
    if 0 in image.shape:
        raise ValueError(f"empty {name}")
    return (T,) + tuple(np.ascontiguousarray(np.swapaxes(a, -3, -2)) for a in (image, features))


def _lens_arrays(lens_radii, focus_dists, n):
    """per-view arrays (None: the keyword for every view) -> two ctypes arrays of n doubles, or None"""
    out = []
    for name, a in (("lens_radii", lens_radii), ("focus_dists", focus_dists)):
        if a is None:
            out.append(None)
            continue
        a = [float(x) for x in a]
        if len(a) != n:
            raise ValueError(f"{len(a)} {name} for {n} views")
        out.append((C.c_double * n)(*a))
    return out


def _stage_host(entry, make, image, features, cam, params):
    """one view on host arrays through ``entry`` (rtw_defocus_ / rtw_wide_aperture_) with the parameters ``make(**params)``"""
    T, img, feat = _host_arrays(image, features)
    W, H = img.shape[:2]
    Cm = _camera_arg(cam, T.type, "cam")
    out = np.empty((W, H, 3), dtype=T)
    _capi.check(_entry(entry, T)(C.byref(make(**params)), C.byref(Cm), W, H, *(a.ctypes.data_as(C.c_void_p) for a in (img, feat, out))))
    return np.swapaxes(out, 0, 1)


def _stage_into(entry, make, d_out_ptr, d_work_ptr, d_image_ptr, d_features_ptr, cam, image_width, image_height, elem_type, stream, params):
    """one view on device pointers through ``entry`` (rtw_defocus_device_ / rtw_wide_aperture_device_)"""
    T = np.dtype(elem_type).type
    Cm = _camera_arg(cam, T, "cam")
    _capi.check(_entry(entry, T)(C.byref(make(**params)), C.byref(Cm), int(image_width), int(image_height),
                                 *(C.c_void_p(int(q)) for q in (d_image_ptr, d_features_ptr, d_work_ptr, d_out_ptr)), C.c_void_p(int(stream))))


def _render_lens(entry, make, word, stage, scene, cams, image_width, n_samples, depth, seed, n_chunks, device, gamma, denoise, batch=None):
    """the one-call body through ``entry`` (rtw_render_defocused_ / rtw_render_wide_aperture_ / rtw_render_lens_batch_): the checks of the
    ``denoise`` and the stage's keywords (``stage``: the dict, ``word``: its name in messages), scene, params, call, stats, reshape.
    ``batch``: None -- ``cams`` is ONE Camera, -> img[i, j, :]; (seeds, lens_radii, focus_dists) -- N cameras, -> img[v, i, j, :]"""
    if batch is None:
        if not isinstance(cams, Camera):
            raise TypeError("cam must be a Camera")
        T = cams.elem_type
    else:
        cams, T = _batch_cameras(cams)
    n = 1 if batch is None else len(cams)
    dk = {} if denoise in (None, False, True) else dict(denoise)
    if set(dk) - set(_DENOISE_KEYS):
        raise ValueError(f"denoise takes the keywords {_DENOISE_KEYS}, got {sorted(set(dk) - set(_DENOISE_KEYS))}")
    bk = {} if stage is None else dict(stage)
    if set(bk) - set(_DEFOCUS_KEYS):
        raise ValueError(f"{word} takes the keywords {_DEFOCUS_KEYS}, got {sorted(set(bk) - set(_DEFOCUS_KEYS))}")
    bk.setdefault("lens_radius", -1.0)                       # (the one-call forms alone: the camera's own)
    if batch is None:
        views, lenses = (C.byref(_capi.make_camera(cams, T)),), ()
    else:
        lenses = tuple(_lens_arrays(batch[1], batch[2], n))
        views = (_capi.make_cameras(cams, T), n, _capi.make_seeds(seed if batch[0] is None else batch[0], n))
    height = _frame_height(image_width, n_samples)
    L = _capi.lib()
    flat = scene if isinstance(scene, dict) else flatten_scene(scene, T)
    S, keep = _capi.make_scene(flat, T)
    P = _capi.make_params(image_width, height, n_samples, depth, seed, n_chunks, 0, 1, device, 1 if gamma else 0, 0)
    D = make_denoise(gamma=gamma, **dk) if denoise else None
    B = make(gamma=gamma, **bk)
    out = np.empty(n * height * int(image_width) * 3, dtype=T)
    _capi.check(_entry(entry, T)(C.byref(S), *views, C.byref(P), C.byref(D) if D is not None else None, C.byref(B), *lenses, out.ctypes.data_as(C.c_void_p)))
    del keep
    _record_stats(L)
    img = out.reshape(n, int(image_width), height, 3).transpose(0, 2, 1, 3)
    return img[0] if batch is None else img


def defocus(image, features, cam, **params):
    """The stage on host arrays (rtw_defocus_*): ``image`` [H, W, 3] (linear, rendered through the pinhole) and ``features`` [H, W, 8] -- or
    the dict ``render_features`` returns -- of the frame seen through ``cam``, whose own ``lens_radius`` is not read: the aperture is the
    keyword.  -> the defocused image [H, W, 3]; a pixel that is not valid is NaN.  Keywords: ``make_defocus``.  Blocking."""
    return _stage_host("rtw_defocus_", make_defocus, image, features, cam, params)


def defocus_into(d_out_ptr, d_work_ptr, d_image_ptr, d_features_ptr, cam, image_width, image_height, *, elem_type=np.float32, stream=0, **params):
    """The device-resident stage (rtw_defocus_device_*): two launches on ``stream``.  DEVICE pointers in the library's layout (pixel (i, j) at
    slot ``j*H + i``): the linear image and the features; ``d_work_ptr``: ``defocus_work_bytes`` bytes, 16-byte aligned, which afterwards hold
    the CoC plane and the tile plane; ``d_out_ptr`` aliases nothing.  Keywords: ``make_defocus``."""
    _stage_into("rtw_defocus_device_", make_defocus, d_out_ptr, d_work_ptr, d_image_ptr, d_features_ptr, cam, image_width, image_height, elem_type, stream, params)


def render_defocused(scene, cam, image_width=400, n_samples=1, *, depth=16, seed=1, n_chunks=0, device=-1, gamma=True, denoise=None, defocus=None):
    """Render through the pinhole and apply the lens afterwards, in one call on the device (rtw_render_defocused_*).  ``cam`` is the camera as
    the user built it, with its aperture: the render and the feature pass run through a copy with ``lens_radius = 0``, the filter follows if
    ``denoise`` is True or a dict of ``make_denoise``'s keywords ``levels, normal_power_log2, sigma_color, sigma_depth, demodulate``, and the
    defocus stage ends the chain; ``defocus``: None, or a dict of ``make_defocus``'s keywords ``lens_radius`` (default: the camera's own),
    ``focus_dist``, ``max_radius``.  Returns ``img[i, j, :]`` -- on the bits the chain of the single calls on the pinhole copy followed by
    ``defocus``; ``last_stats()`` reports the render."""
    return _render_lens("rtw_render_defocused_", make_defocus, "defocus", defocus, scene, cam, image_width, n_samples, depth, seed, n_chunks, device, gamma, denoise)
