"""First-hit feature buffers (include/rtw_hip.h ``rtw_render_features_*``): per pixel the albedo, the normal, the depth and the
coverage of what the camera sees first -- the guides a denoiser, an edge-aware upsampler or a compositing step wants next to a
low-sample-count image.

The feature sample of (pixel, chunk) is the primary ray of the chunk's first sample of the render ``(image_width, n_samples, seed,
n_chunks, numerics)`` describes, so the buffers belong to that render's image -- or, with ``chunks=(begin, count)``, to the progressive
passes over those chunks.  Sums are exact (64.64 fixed point): the result does not depend on the scan mode or the launch shape.
Normals are not renormalised and depth is averaged over all samples: divide both by ``coverage``.  All compute happens in
librtw_hip.so; there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _capi
from .render import _batch_cameras, _frame_height, _record_stats      # (last_stats() reports the feature pass too)
from .structs import flatten_scene

FEATURE_CHANNELS = 8     # include/rtw_hip.h RTW_FEATURE_CHANNELS


def _elem_type(cam, elem_type):
    T = cam.elem_type if elem_type is None else elem_type
    if np.dtype(T) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("elem_type must be float32 or float64")
    return np.dtype(T).type


def _params(image_width, n_samples, seed, n_chunks, device, numerics, flags, job_pixels=0):
    height = _frame_height(image_width, n_samples)
    # (max_depth and gamma are ignored by the feature pass: the render's defaults keep the struct valid)
    return height, _capi.make_params(image_width, height, n_samples, 16, seed, n_chunks, 0, 1, device, 1, flags,
                                     job_pixels=job_pixels, numerics=numerics)


def effective_chunks(n_samples, n_chunks=0):
    """N: the effective chunks of a render under the default rule of rtw_params.n_chunks -> (N, chunk size s)"""
    nch = int(n_chunks) if int(n_chunks) > 0 else min(int(n_samples), 256)
    nch = min(nch, int(n_samples))
    s = -(-int(n_samples) // nch)
    return -(-int(n_samples) // s), s


def _range(chunks, n_samples, n_chunks):
    if chunks is None:
        return 0, effective_chunks(n_samples, n_chunks)[0]
    begin, count = chunks
    return int(begin), int(count)


def split(raw):
    """``raw[i, j, 8]`` -> the dict ``render_features`` returns (views of ``raw``)"""
    return {"albedo": raw[..., 0:3], "normal": raw[..., 3:6], "depth": raw[..., 6], "coverage": raw[..., 7], "raw": raw}


def _host_features(scene, T, Cm, n, sd, image_width, n_samples, seed, n_chunks, chunks, device, numerics, flags):
    """Both host-buffer calls behind their camera checks -> raw [max(n, 1), H, W, 8].  n == 0: rtw_render_features_* through the one
    camera ``Cm``; n >= 1: rtw_render_features_batch_* through the n cameras ``Cm`` with the seeds ``sd``."""
    L = _capi.lib()
    height, P = _params(image_width, n_samples, seed, n_chunks, device, numerics, flags)
    begin, count = _range(chunks, n_samples, n_chunks)
    flat = scene if isinstance(scene, dict) else flatten_scene(scene, T)
    S, keep = _capi.make_scene(flat, T)
    out = np.empty(max(n, 1) * height * int(image_width) * FEATURE_CHANNELS, dtype=T)
    sfx = "f64" if _capi.is_f64(T) else "f32"
    if n:
        rc = getattr(L, "rtw_render_features_batch_" + sfx)(C.byref(S), Cm, n, sd, C.byref(P), begin, count, out.ctypes.data_as(C.c_void_p))
    else:
        rc = getattr(L, "rtw_render_features_" + sfx)(C.byref(S), C.byref(Cm), C.byref(P), begin, count, out.ctypes.data_as(C.c_void_p))
    _capi.check(rc)
    del keep
    _record_stats(L)
    return out.reshape(max(n, 1), int(image_width), height, FEATURE_CHANNELS).transpose(0, 2, 1, 3)


def _features_into(renderer, d_out_ptr, Cm, n, sd, image_width, n_samples, seed, n_chunks, chunks, stream, flags, job_pixels, numerics, n_elems):
    """Both device-resident calls (``n`` as in ``_host_features``).  Returns H."""
    height, P = _params(image_width, n_samples, seed, n_chunks, -1, numerics, flags, job_pixels)
    need = max(n, 1) * height * int(image_width) * FEATURE_CHANNELS
    if n_elems is not None and int(n_elems) < need:
        raise ValueError(f"output buffer holds {n_elems} elements, the {'batched ' if n else ''}feature pass writes {need}")
    begin, count = _range(chunks, n_samples, n_chunks)
    L = renderer.L
    sfx = "f64" if _capi.is_f64(renderer.T) else "f32"
    if n:
        rc = getattr(L, "rtw_render_features_batch_device_" + sfx)(renderer.handle, Cm, n, sd, C.byref(P), begin, count, C.c_void_p(int(d_out_ptr)),
                                                                 C.c_void_p(int(stream)))
    else:
        rc = getattr(L, "rtw_render_features_device_" + sfx)(renderer.handle, C.byref(Cm), C.byref(P), begin, count, C.c_void_p(int(d_out_ptr)),
                                                           C.c_void_p(int(stream)))
    _capi.check(rc)
    return height


def render_features(scene, cam, image_width=400, n_samples=1, *, seed=1, n_chunks=0, chunks=None, device=-1, numerics=None, flags=0,
                    elem_type=None):
    """First-hit features of the render ``render(scene, cam, image_width, n_samples, seed=seed, n_chunks=n_chunks)``: a dict of
    ``albedo`` [H, W, 3], ``normal`` [H, W, 3], ``depth`` [H, W], ``coverage`` [H, W] and ``raw`` [H, W, 8] (the others are views of it),
    of the camera's element type (``elem_type`` overrides it).  ``chunks=None``: the whole render; ``chunks=(begin, count)``: that range of
    its effective chunks.  ``scene``: a HittableList or the flat dict of ``flatten_scene``.  ``flags``: RTW_FLAG_GROUP_CULL /
    RTW_FLAG_SCAN_VALU are accepted and change nothing."""
    T = _elem_type(cam, elem_type)
    return split(_host_features(scene, T, _capi.make_camera(cam, T), 0, None, image_width, n_samples, seed, n_chunks, chunks, device, numerics, flags)[0])


def features_into(renderer, d_out_ptr, image_width, n_samples, *, seed=1, n_chunks=0, chunks=None, stream=0, flags=0, job_pixels=0,
                  numerics=None, n_elems=None):
    """The device-resident form (rtw_render_features_device_*; ``DeviceRenderer.features_into``): enqueue the feature pass of
    ``renderer``'s scene and camera into device memory at ``d_out_ptr`` -- H*W*8 elements, 16-byte aligned, pixel (i, j) at
    ``(j*H + i) * 8`` (0-based) -- on ``stream``.  ``n_elems``: the buffer's length in elements; checked when given.  Returns H."""
    return _features_into(renderer, d_out_ptr, renderer.cam, 0, None, image_width, n_samples, seed, n_chunks, chunks, stream, flags, job_pixels, numerics, n_elems)


def render_features_batch(scene, cams, image_width=400, n_samples=1, *, seeds=None, seed=1, n_chunks=0, chunks=None, device=-1, numerics=None,
                          flags=0):
    """The feature buffers of N views of ``scene`` in ONE launch (rtw_render_features_batch_*): the dict of ``render_features`` with a
    leading view axis -- ``raw`` [N, H, W, 8], ``albedo`` [N, H, W, 3], ... -- the way ``render_batch`` stacks its frames.  View ``v`` is
    bit for bit ``render_features(scene, cams[v], ..., seed=seeds[v])``.  ``seeds``: a sequence of ``len(cams)`` ints (None: ``seed`` for
    every view).  Same size, spp, chunks and mode for every view; one device."""
    cams, T = _batch_cameras(cams)
    sd = _capi.make_seeds(seed if seeds is None else seeds, len(cams))
    return split(_host_features(scene, T, _capi.make_cameras(cams, T), len(cams), sd, image_width, n_samples, seed, n_chunks, chunks, device, numerics, flags))


def features_batch_into(renderer, d_out_ptr, cams, image_width, n_samples, *, seeds=None, seed=1, n_chunks=0, chunks=None, stream=0, flags=0,
                        job_pixels=0, numerics=None, n_elems=None):
    """The device-resident batched form (rtw_render_features_batch_device_*; ``DeviceRenderer.features_batch_into``): enqueue ONE feature
    launch of ``renderer``'s scene through ``cams`` into device memory at ``d_out_ptr`` -- len(cams) consecutive buffers of H*W*8
    elements, 16-byte aligned -- on ``stream``.  ``n_elems``: the buffer's length in elements; checked when given.  Returns H."""
    cams, T = _batch_cameras(cams)
    if np.dtype(T) != np.dtype(renderer.T):
        raise TypeError("the cameras' elem_type differs from the scene's")
    sd = _capi.make_seeds(seed if seeds is None else seeds, len(cams))
    return _features_into(renderer, d_out_ptr, _capi.make_cameras(cams, T), len(cams), sd, image_width, n_samples, seed, n_chunks, chunks, stream, flags,
                          job_pixels, numerics, n_elems)
