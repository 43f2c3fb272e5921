"""Feature-guided denoiser (include/rtw_hip.h ``rtw_denoise_*``): an edge-avoiding a-trous filter of a low-sample-count image -- a
progressive prefix, an adaptive render that stopped early, a 1-4 spp preview -- guided by the first-hit feature buffers of
``render_features``.  The definition is in the header; tests/denoise_ref.py restates it on the CPU and the device agrees on the bits.
All compute happens in librtw_hip.so; there is no CPU fallback.

Defaults: ``levels=3, normal_power_log2=1, sigma_color=0.5, sigma_depth=0.1, demodulate=True, gamma=True``.  The image handed in is
normally a LINEAR one (``render(..., gamma=False)``): the denoiser applies gamma itself at the end.
"""
import ctypes as C

import numpy as np

from . import _capi
from .render import _batch_cameras, _frame_height, _record_stats
from .structs import Camera, flatten_scene


#: Default ``sigma_color`` of the noise-guided form (``AdaptiveRenderer.denoised``, ``denoise_guided_into``): there it counts estimated
#: standard deviations of the pixel.  Measured on the CPU witness (the power of two with the lowest MSE).
GUIDED_SIGMA_COLOR = 1.0


def make_denoise(levels=3, normal_power_log2=1, sigma_color=0.5, sigma_depth=0.1, demodulate=True, gamma=True, device=-1):
    """-> the ``rtw_denoise_t`` of these keywords"""
    flags = _capi.DENOISE_DEMODULATE if demodulate else 0
    return _capi.Denoise(int(levels), int(normal_power_log2), flags, 1 if gamma else 0, int(device), 0, float(sigma_color), float(sigma_depth))


def denoise_work_bytes(image_width, image_height, elem_type=np.float32):
    """bytes of device workspace ``denoise_into`` needs for one frame (16-byte aligned, owned by the caller)"""
    n = _capi.lib().rtw_denoise_work_bytes(int(image_width), int(image_height), np.dtype(elem_type).itemsize)
    if n < 0:
        _capi.check(int(n))
    return int(n)


def _filter_host(images, features, batch, params):
    """``denoise`` (one frame: [H, W, .]) and ``denoise_batch`` ([N, H, W, .]): one set of checks, one call, the result in the inputs' shape"""
    if isinstance(features, dict):
        features = features["raw"]
    images, features = np.asarray(images), np.asarray(features)
    T = images.dtype
    name, dims = ("images", "[N, H, W, ") if batch else ("image", "[H, W, ")
    if T not in (np.dtype(np.float32), np.dtype(np.float64)) or features.dtype != T:
        raise TypeError(f"{name} and features must both be float32 or both float64")
    if images.ndim != (4 if batch else 3) or images.shape[-1] != 3 or features.shape != images.shape[:-1] + (8,):
        raise ValueError(f"expected {name} {dims}3] and features {dims}8], got {images.shape} and {features.shape}")
    if 0 in images.shape:
        raise ValueError("empty batch" if batch else "empty image")
    H, W = images.shape[-3:-1]
    D = make_denoise(**params)
    img = np.ascontiguousarray(np.swapaxes(images, -3, -2))         # the library's layout: view v, pixel (i, j) at v*W*H + j*H + i
    feat = np.ascontiguousarray(np.swapaxes(features, -3, -2))
    out = np.empty(img.shape, dtype=T)
    ptrs = [a.ctypes.data_as(C.c_void_p) for a in (img, feat, out)]
    L = _capi.lib()
    sfx = "f64" if _capi.is_f64(T) else "f32"
    if batch:
        _capi.check(getattr(L, "rtw_filter_batch_" + sfx)(C.byref(D), W, H, images.shape[0], *ptrs))
    else:
        _capi.check(getattr(L, "rtw_denoise_" + sfx)(C.byref(D), W, H, *ptrs))
    return np.swapaxes(out, -3, -2)


def denoise(image, features, **params):
    """``image`` [H, W, 3] and ``features`` [H, W, 8] -- or the dict ``render_features`` returns -- host arrays of one element type
    (float32 / float64) -> the denoised image [H, W, 3].  Keywords: ``make_denoise``.  Blocking; ``last_stats()`` is left as it was."""
    return _filter_host(image, features, False, params)


def _filter_into(entry, frames, what, ptrs, image_width, image_height, elem_type, stream, work_bytes, params, n_views=()):
    """The three device-resident forms: the workspace check for ``frames`` frames, ``make_denoise`` and the call of ``entry`` + f32 / f64"""
    need = frames * denoise_work_bytes(image_width, image_height, elem_type)
    if work_bytes is not None and int(work_bytes) < need:
        raise ValueError(f"workspace holds {work_bytes} bytes, the {what} needs {need}")
    D = make_denoise(**params)
    fn = getattr(_capi.lib(), entry + ("f64" if _capi.is_f64(elem_type) else "f32"))
    _capi.check(fn(C.byref(D), int(image_width), int(image_height), *n_views, *(C.c_void_p(int(q)) for q in ptrs), C.c_void_p(int(stream))))


def denoise_into(d_out_ptr, d_image_ptr, d_features_ptr, d_work_ptr, image_width, image_height, *, elem_type=np.float32, stream=0,
                 work_bytes=None, **params):
    """The device-resident form (rtw_denoise_device_*): enqueue the denoiser on ``stream``.  All four are DEVICE pointers (a torch
    tensor's ``data_ptr()``): the image and the result hold H*W*3 elements, the features H*W*8 (16-byte aligned), the workspace
    ``denoise_work_bytes(...)`` bytes (16-byte aligned; ``work_bytes``: its size, checked when given).  The result may not alias an
    input or the workspace; concurrent calls need a workspace each.  Keywords: ``make_denoise``."""
    _filter_into("rtw_denoise_device_", 1, "denoiser", (d_image_ptr, d_features_ptr, d_out_ptr, d_work_ptr), image_width, image_height, elem_type, stream,
                 work_bytes, params)


def denoise_guided_into(d_out_ptr, d_image_ptr, d_features_ptr, d_noise_ptr, d_work_ptr, image_width, image_height, *, elem_type=np.float32,
                        stream=0, work_bytes=None, **params):
    """The noise-guided device form (rtw_guided_filter_device_*): ``denoise_into`` with one more input, ``d_noise_ptr``: H*W elements,
    the per-pixel relative noise (``AdaptiveRenderer.noise_into``).  ``sigma_color`` defaults to ``GUIDED_SIGMA_COLOR``."""
    params.setdefault("sigma_color", GUIDED_SIGMA_COLOR)
    _filter_into("rtw_guided_filter_device_", 1, "denoiser", (d_image_ptr, d_features_ptr, d_noise_ptr, d_out_ptr, d_work_ptr), image_width, image_height,
                 elem_type, stream, work_bytes, params)


def _render_filtered(scene, T, Cm, n, sd, image_width, n_samples, depth, seed, n_chunks, device, gamma, group_cull, scan_valu, numerics, dn):
    """Both one-call forms behind their camera checks -> img [max(n, 1), H, W, 3].  n == 0: rtw_render_denoised_* through the one camera
    ``Cm``; n >= 1: rtw_render_filtered_batch_* through the n cameras ``Cm`` with the seeds ``sd``.  ``dn``: ``make_denoise``'s first five."""
    height = _frame_height(image_width, n_samples)
    L = _capi.lib()
    flat = scene if isinstance(scene, dict) else flatten_scene(scene, T)
    S, keep = _capi.make_scene(flat, T)
    P = _capi.make_params(image_width, height, n_samples, depth, seed, n_chunks, 0, 1, device, 1 if gamma else 0,
                          (_capi.FLAG_GROUP_CULL if group_cull else 0) | (_capi.FLAG_SCAN_VALU if scan_valu else 0), numerics=numerics)
    D = make_denoise(*dn, gamma)
    out = np.empty(max(n, 1) * height * int(image_width) * 3, dtype=T)
    sfx = "f64" if _capi.is_f64(T) else "f32"
    if n:
        rc = getattr(L, "rtw_render_filtered_batch_" + sfx)(C.byref(S), Cm, n, sd, C.byref(P), C.byref(D), out.ctypes.data_as(C.c_void_p))
    else:
        rc = getattr(L, "rtw_render_denoised_" + sfx)(C.byref(S), C.byref(Cm), C.byref(P), C.byref(D), out.ctypes.data_as(C.c_void_p))
    _capi.check(rc)
    del keep
    _record_stats(L)
    return out.reshape(max(n, 1), int(image_width), height, 3).transpose(0, 2, 1, 3)


def render_denoised(scene, cam, image_width=400, n_samples=1, *, depth=16, seed=1, n_chunks=0, device=-1, gamma=True, group_cull=False,
                    scan_valu=False, numerics=None, levels=3, normal_power_log2=1, sigma_color=0.5, sigma_depth=0.1, demodulate=True):
    """``render`` + ``render_features`` + ``denoise`` in one call on the device (rtw_render_denoised_*): the linear image, the feature
    pass over all of its chunks and the filter stay in HBM, the result comes back once.  Returns ``img[i, j, :]``; ``last_stats()``
    reports the render."""
    if not isinstance(cam, Camera):
        raise TypeError("cam must be a Camera")
    T = cam.elem_type
    return _render_filtered(scene, T, _capi.make_camera(cam, T), 0, None, image_width, n_samples, depth, seed, n_chunks, device, gamma, group_cull, scan_valu,
                            numerics, (levels, normal_power_log2, sigma_color, sigma_depth, demodulate))[0]


def denoise_batch(images, features, **params):
    """``images`` [N, H, W, 3] and ``features`` [N, H, W, 8] -- or the dict ``render_features_batch`` returns -- -> the N denoised images
    [N, H, W, 3] in prepare + ``levels`` launches for all views (rtw_filter_batch_*).  View ``v`` is bit for bit
    ``denoise(images[v], features[v], ...)``.  Keywords: ``make_denoise``.  Blocking; ``last_stats()`` is left as it was."""
    return _filter_host(images, features, True, params)


def denoise_batch_into(d_out_ptr, d_images_ptr, d_features_ptr, d_work_ptr, image_width, image_height, n_views, *, elem_type=np.float32,
                       stream=0, work_bytes=None, **params):
    """The device-resident batched form (rtw_filter_batch_device_*): ``denoise_into`` for ``n_views`` frames one behind the other in
    every buffer.  The workspace holds ``n_views * denoise_work_bytes(...)`` bytes (``work_bytes``: its size, checked when given); its
    planes are batch-major, so it is one workspace, not ``n_views`` single-frame ones.  Keywords: ``make_denoise``."""
    if int(n_views) < 1:
        raise ValueError("n_views must be >= 1")
    _filter_into("rtw_filter_batch_device_", int(n_views), "batched filter", (d_images_ptr, d_features_ptr, d_out_ptr, d_work_ptr), image_width, image_height,
                 elem_type, stream, work_bytes, params, n_views=(int(n_views),))


def denoise_guided_batch_into(d_out_ptr, d_images_ptr, d_features_ptr, d_noise_ptr, d_work_ptr, image_width, image_height, n_views, *,
                              elem_type=np.float32, stream=0, work_bytes=None, **params):
    """The noise-guided batched device form (rtw_guided_filter_batch_device_*): ``denoise_batch_into`` with one more input,
    ``d_noise_ptr``: n_views*H*W elements, view ``v``'s map at ``v*H*W`` (``AdaptiveBatchRenderer.noise_all_into``).  View ``v`` is bit for
    bit ``denoise_guided_into`` on frame ``v``.  ``sigma_color`` defaults to ``GUIDED_SIGMA_COLOR``."""
    if int(n_views) < 1:
        raise ValueError("n_views must be >= 1")
    params.setdefault("sigma_color", GUIDED_SIGMA_COLOR)
    _filter_into("rtw_guided_filter_batch_device_", int(n_views), "batched filter", (d_images_ptr, d_features_ptr, d_noise_ptr, d_out_ptr, d_work_ptr),
                 image_width, image_height, elem_type, stream, work_bytes, params, n_views=(int(n_views),))


def render_denoised_batch(scene, cams, image_width=400, n_samples=1, *, seeds=None, depth=16, seed=1, n_chunks=0, device=-1, gamma=True,
                          group_cull=False, scan_valu=False, numerics=None, levels=3, normal_power_log2=1, sigma_color=0.5, sigma_depth=0.1,
                          demodulate=True):
    """``render_batch`` + ``render_features_batch`` + ``denoise_batch`` in one call on the device (rtw_render_filtered_batch_*):
    2 + 1 + ``levels`` launches for any number of views, the result comes back once.  Returns ``img[v, i, j, :]``; view ``v`` is bit for
    bit ``render_denoised(scene, cams[v], ..., seed=seeds[v])``.  ``seeds``: a sequence of ``len(cams)`` ints (None: ``seed`` for every
    view).  ``last_stats()`` reports the render."""
    cams, T = _batch_cameras(cams)
    sd = _capi.make_seeds(seed if seeds is None else seeds, len(cams))
    return _render_filtered(scene, T, _capi.make_cameras(cams, T), len(cams), sd, image_width, n_samples, depth, seed, n_chunks, device, gamma, group_cull,
                            scan_valu, numerics, (levels, normal_power_log2, sigma_color, sigma_depth, demodulate))
