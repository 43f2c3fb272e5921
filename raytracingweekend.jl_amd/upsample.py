"""Feature-guided upsampler (include/rtw_hip.h ``rtw_upsample_*``): a full-size frame from a small render.  The small image is
prepared and filtered like the denoiser's (``levels`` a-trous passes at the small size), then every full-size pixel gathers 4 x 4 small
pixels under weights from its OWN full-size feature buffer (albedo, coverage, normal, depth), so silhouettes and albedo detail come from
the full frame.  The definition is in the header; tests/upsample_ref.py restates it on the CPU and the device agrees on the bits.  All
compute happens in librtw_hip.so; there is no CPU fallback.

Defaults: ``levels=2, normal_power_log2=1, sigma_color=0.5, sigma_depth=0.1, sigma_albedo=0.2, demodulate=True, gamma=True``.  They are
UNTUNED: the first four are the denoiser's, and 0.2 for ``sigma_albedo`` comes from a synthetic numpy prototype, not from a render.
The small image handed in is normally a LINEAR one (``render(..., gamma=False)``): the upsampler applies gamma itself at the end.
"""
import ctypes as C

import numpy as np

from . import _capi
from .render import _batch_cameras, _frame_height, _record_stats
from .structs import Camera, flatten_scene, image_height


def make_upsample(levels=2, normal_power_log2=1, sigma_color=0.5, sigma_depth=0.1, sigma_albedo=0.2, demodulate=True, gamma=True, device=-1,
                  hi_chunks=0):
    """-> the ``rtw_upsample_t`` of these keywords (the defaults are untuned: see the module's docstring)"""
    flags = _capi.UPSAMPLE_DEMODULATE if demodulate else 0
    return _capi.Upsample(int(levels), int(normal_power_log2), flags, 1 if gamma else 0, int(device), int(hi_chunks), float(sigma_color),
                          float(sigma_depth), float(sigma_albedo))


def upsample_work_bytes(lo_width, lo_height, elem_type=np.float32):
    """bytes of device workspace ``upsample_into`` needs for one view: the denoiser's for the SMALL frame (16-byte aligned, owned by the caller)"""
    n = _capi.lib().rtw_upsample_work_bytes(int(lo_width), int(lo_height), np.dtype(elem_type).itemsize)
    if n < 0:
        _capi.check(int(n))
    return int(n)


def _upsample_host(images_lo, features_lo, features_hi, batch, params):
    """``upsample`` (one view: [h, w, .] and [H, W, 8]) and ``upsample_batch`` ([N, ...]): one set of checks, one call"""
    features_lo = features_lo["raw"] if isinstance(features_lo, dict) else features_lo
    features_hi = features_hi["raw"] if isinstance(features_hi, dict) else features_hi
    images_lo, features_lo, features_hi = np.asarray(images_lo), np.asarray(features_lo), np.asarray(features_hi)
    T = images_lo.dtype
    nd = 4 if batch else 3
    if T not in (np.dtype(np.float32), np.dtype(np.float64)) or features_lo.dtype != T or features_hi.dtype != T:
        raise TypeError("the small image and both feature buffers must all be float32 or all float64")
    if images_lo.ndim != nd or images_lo.shape[-1] != 3 or features_lo.shape != images_lo.shape[:-1] + (8,) or features_hi.ndim != nd or \
            features_hi.shape[-1] != 8 or (batch and features_hi.shape[0] != images_lo.shape[0]):
        lead = "[N, " if batch else "["
        raise ValueError(f"expected a small image {lead}h, w, 3], small features {lead}h, w, 8] and full features {lead}H, W, 8], got "
                         f"{images_lo.shape}, {features_lo.shape} and {features_hi.shape}")
    if 0 in images_lo.shape or 0 in features_hi.shape:
        raise ValueError("empty batch" if batch else "empty image")
    h, w = images_lo.shape[-3:-1]
    H, W = features_hi.shape[-3:-1]
    if w > W or h > H:
        raise ValueError(f"the small frame {w} x {h} exceeds the full frame {W} x {H}")
    U = make_upsample(**params)
    img = np.ascontiguousarray(np.swapaxes(images_lo, -3, -2))      # the library's layout: view v, pixel (i, j) at (v*cols + j)*rows + i
    flo = np.ascontiguousarray(np.swapaxes(features_lo, -3, -2))
    fhi = np.ascontiguousarray(np.swapaxes(features_hi, -3, -2))
    out = np.empty(fhi.shape[:-1] + (3,), dtype=T)
    ptrs = [a.ctypes.data_as(C.c_void_p) for a in (img, flo, fhi, out)]
    L = _capi.lib()
    sfx = "f64" if _capi.is_f64(T) else "f32"
    if batch:
        _capi.check(getattr(L, "rtw_upsample_batch_" + sfx)(C.byref(U), w, h, W, H, images_lo.shape[0], *ptrs))
    else:
        _capi.check(getattr(L, "rtw_upsample_" + sfx)(C.byref(U), w, h, W, H, *ptrs))
    return np.swapaxes(out, -3, -2)


def upsample(image_lo, features_lo, features_hi, **params):
    """``image_lo`` [h, w, 3] and ``features_lo`` [h, w, 8] of the small frame, ``features_hi`` [H, W, 8] of the full one -- arrays or the
    dicts ``render_features`` returns, all of one element type (float32 / float64) -> the full-size image [H, W, 3].  Keywords:
    ``make_upsample``.  Blocking; ``last_stats()`` is left as it was."""
    return _upsample_host(image_lo, features_lo, features_hi, False, params)


def upsample_batch(images_lo, features_lo, features_hi, **params):
    """``images_lo`` [N, h, w, 3], ``features_lo`` [N, h, w, 8], ``features_hi`` [N, H, W, 8] -> the N full-size images [N, H, W, 3] in
    prepare + ``levels`` + 1 launches for all views (rtw_upsample_batch_*).  View ``v`` is bit for bit ``upsample`` of its frames."""
    return _upsample_host(images_lo, features_lo, features_hi, True, params)


def _upsample_into(entry, frames, ptrs, lo_width, lo_height, image_width, image_height_, elem_type, stream, work_bytes, params, n_views=()):
    need = frames * upsample_work_bytes(lo_width, lo_height, elem_type)
    if work_bytes is not None and int(work_bytes) < need:
        raise ValueError(f"workspace holds {work_bytes} bytes, the upsampler needs {need}")
    U = make_upsample(**params)
    fn = getattr(_capi.lib(), entry + ("f64" if _capi.is_f64(elem_type) else "f32"))
    _capi.check(fn(C.byref(U), int(lo_width), int(lo_height), int(image_width), int(image_height_), *n_views, *(C.c_void_p(int(q)) for q in ptrs),
                   C.c_void_p(int(stream))))


def upsample_into(d_out_ptr, d_image_lo_ptr, d_features_lo_ptr, d_features_hi_ptr, d_work_ptr, lo_width, lo_height, image_width, image_height, *,
                  elem_type=np.float32, stream=0, work_bytes=None, **params):
    """The device-resident form (rtw_upsample_device_*): enqueue the upsampler on ``stream``.  All five are DEVICE pointers: the small
    image h*w*3 elements, the small features h*w*8 and the full features H*W*8 (both 16-byte aligned), the result H*W*3, the workspace
    ``upsample_work_bytes(lo_width, lo_height, ...)`` bytes (16-byte aligned; ``work_bytes``: its size, checked when given).  The result
    aliases nothing, the workspace no input; concurrent calls need a workspace each.  Keywords: ``make_upsample``."""
    _upsample_into("rtw_upsample_device_", 1, (d_image_lo_ptr, d_features_lo_ptr, d_features_hi_ptr, d_out_ptr, d_work_ptr), lo_width, lo_height, image_width,
                   image_height, elem_type, stream, work_bytes, params)


def upsample_batch_into(d_out_ptr, d_images_lo_ptr, d_features_lo_ptr, d_features_hi_ptr, d_work_ptr, lo_width, lo_height, image_width, image_height,
                        n_views, *, elem_type=np.float32, stream=0, work_bytes=None, **params):
    """The device-resident batched form (rtw_upsample_batch_device_*): ``upsample_into`` for ``n_views`` views one behind the other in every
    buffer, each at its own frame size.  The workspace holds ``n_views * upsample_work_bytes(...)`` bytes; its planes are batch-major."""
    if int(n_views) < 1:
        raise ValueError("n_views must be >= 1")
    _upsample_into("rtw_upsample_batch_device_", int(n_views), (d_images_lo_ptr, d_features_lo_ptr, d_features_hi_ptr, d_out_ptr, d_work_ptr), lo_width,
                   lo_height, image_width, image_height, elem_type, stream, work_bytes, params, n_views=(int(n_views),))


def _render_upsampled(scene, T, Cm, n, sd, image_width, n_samples, lo_width, depth, seed, n_chunks, device, gamma, group_cull, scan_valu, numerics, up):
    """Both one-call forms behind their camera checks -> img [max(n, 1), H, W, 3].  n == 0: rtw_render_upsampled_* through the one camera
    ``Cm``; n >= 1: rtw_render_upsampled_batch_* through the n cameras ``Cm`` with the seeds ``sd``.  ``up``: ``make_upsample``'s keywords."""
    height = _frame_height(image_width, n_samples)
    lo_width = (int(image_width) + 1) // 2 if lo_width is None else int(lo_width)
    lo_height = image_height(lo_width)
    if not (1 <= lo_width <= int(image_width)) or lo_height < 1:
        raise ValueError(f"lo_width={lo_width} gives a small frame {lo_width} x {lo_height} for the full frame {image_width} x {height}")
    L = _capi.lib()
    flat = scene if isinstance(scene, dict) else flatten_scene(scene, T)
    S, keep = _capi.make_scene(flat, T)
    P = _capi.make_params(image_width, height, n_samples, depth, seed, n_chunks, 0, 1, device, 1 if gamma else 0,
                          (_capi.FLAG_GROUP_CULL if group_cull else 0) | (_capi.FLAG_SCAN_VALU if scan_valu else 0), numerics=numerics)
    U = make_upsample(gamma=gamma, **up)
    out = np.empty(max(n, 1) * height * int(image_width) * 3, dtype=T)
    sfx = "f64" if _capi.is_f64(T) else "f32"
    if n:
        rc = getattr(L, "rtw_render_upsampled_batch_" + sfx)(C.byref(S), Cm, n, sd, C.byref(P), lo_width, lo_height, C.byref(U), out.ctypes.data_as(C.c_void_p))
    else:
        rc = getattr(L, "rtw_render_upsampled_" + sfx)(C.byref(S), C.byref(Cm), C.byref(P), lo_width, lo_height, C.byref(U), out.ctypes.data_as(C.c_void_p))
    _capi.check(rc)
    del keep
    _record_stats(L)
    return out.reshape(max(n, 1), int(image_width), height, 3).transpose(0, 2, 1, 3)


def render_upsampled(scene, cam, image_width=400, n_samples=1, *, lo_width=None, depth=16, seed=1, n_chunks=0, device=-1, gamma=True, group_cull=False,
                     scan_valu=False, numerics=None, hi_chunks=0, levels=2, normal_power_log2=1, sigma_color=0.5, sigma_depth=0.1, sigma_albedo=0.2,
                     demodulate=True):
    """A render at ``lo_width`` (default ``ceil(image_width / 2)``; the small height is ``image_height(lo_width)``), its feature pass, the
    feature pass of the full frame over its first ``hi_chunks`` chunks (0: all) and ``upsample`` in one call on the device
    (rtw_render_upsampled_*): everything stays in HBM, the full-size result comes back once.  Returns ``img[i, j, :]`` of the full size;
    ``last_stats()`` reports the small render.  The filter's defaults are untuned (see the module's docstring)."""
    if not isinstance(cam, Camera):
        raise TypeError("cam must be a Camera")
    T = cam.elem_type
    up = dict(levels=levels, normal_power_log2=normal_power_log2, sigma_color=sigma_color, sigma_depth=sigma_depth, sigma_albedo=sigma_albedo,
              demodulate=demodulate, hi_chunks=hi_chunks)
    return _render_upsampled(scene, T, _capi.make_camera(cam, T), 0, None, image_width, n_samples, lo_width, depth, seed, n_chunks, device, gamma, group_cull,
                             scan_valu, numerics, up)[0]


def render_upsampled_batch(scene, cams, image_width=400, n_samples=1, *, seeds=None, lo_width=None, depth=16, seed=1, n_chunks=0, device=-1, gamma=True,
                           group_cull=False, scan_valu=False, numerics=None, hi_chunks=0, levels=2, normal_power_log2=1, sigma_color=0.5, sigma_depth=0.1,
                           sigma_albedo=0.2, demodulate=True):
    """``render_upsampled`` for N cameras of one scene in 5 + ``levels`` launches (rtw_render_upsampled_batch_*).  Returns
    ``img[v, i, j, :]``; view ``v`` is bit for bit ``render_upsampled(scene, cams[v], ..., seed=seeds[v])``.  ``seeds``: a sequence of
    ``len(cams)`` ints (None: ``seed`` for every view).  ``last_stats()`` reports the small render."""
    cams, T = _batch_cameras(cams)
    sd = _capi.make_seeds(seed if seeds is None else seeds, len(cams))
    up = dict(levels=levels, normal_power_log2=normal_power_log2, sigma_color=sigma_color, sigma_depth=sigma_depth, sigma_albedo=sigma_albedo,
              demodulate=demodulate, hi_chunks=hi_chunks)
    return _render_upsampled(scene, T, _capi.make_cameras(cams, T), len(cams), sd, image_width, n_samples, lo_width, depth, seed, n_chunks, device, gamma,
                             group_cull, scan_valu, numerics, up)
