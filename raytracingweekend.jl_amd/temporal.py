"""Temporal reprojection (include/rtw_hip.h ``rtw_temporal_*``): history reuse along a camera path over one static scene.  A step blends
a frame's linear image with the history the previous frame left, gathered where the pixel's first-hit point lay in the previous view, under
weights from the feature buffers (coverage, normal, depth); the state (accumulated colour, guides, history length) travels from frame to
frame.  The definition is in the header; tests/temporal_ref.py restates it on the CPU and the device agrees on the bits.  All compute happens
in librtw_hip.so; there is no CPU fallback.

Defaults: ``normal_power_log2=1, sigma_depth=0.1, min_weight=0.25, history_max=16, demodulate=True, gamma=True``.  They are UNTUNED beyond a
small grid on the CPU witness.  The image handed to a step is a LINEAR one (``render(..., gamma=False)``): the step
applies gamma itself at the end, and the state stays linear.
"""
import ctypes as C

import numpy as np

from . import _capi
from .denoise import make_denoise
from .render import _batch_cameras, _frame_height, _record_stats
from .structs import Camera

_DENOISE_KEYS = ("levels", "normal_power_log2", "sigma_color", "sigma_depth", "demodulate")


def make_temporal(normal_power_log2=1, sigma_depth=0.1, min_weight=0.25, history_max=16.0, demodulate=True, gamma=True, device=-1):
    """-> the ``rtw_temporal_t`` of these keywords (the defaults are untuned: see the module's docstring)"""
    flags = _capi.TEMPORAL_DEMODULATE if demodulate else 0
    return _capi.Temporal(int(normal_power_log2), flags, 1 if gamma else 0, int(device), (C.c_int32 * 2)(0, 0), float(sigma_depth), float(min_weight),
                          float(history_max))


def temporal_state_bytes(image_width, image_height, elem_type=np.float32):
    """bytes of one state: the planes E (4 per pixel), G (4 per pixel) and L (1 per pixel), 9*W*H elements rounded up to 16 bytes"""
    n = _capi.lib().rtw_temporal_state_bytes(int(image_width), int(image_height), np.dtype(elem_type).itemsize)
    if n < 0:
        _capi.check(int(n))
    return int(n)


def _camera_arg(cam, T, what):
    if not isinstance(cam, Camera):
        raise TypeError(f"{what} must be a Camera")
    if np.dtype(cam.elem_type) != np.dtype(T):
        raise TypeError(f"{what} has element type {np.dtype(cam.elem_type).name}, the frame {np.dtype(T).name}")
    return _capi.make_camera(cam, T)


def temporal_step(image, features, cam, state=None, cam_prev=None, **params):
    """One step on host arrays (rtw_temporal_*): ``image`` [H, W, 3] (linear) and ``features`` [H, W, 8] -- or the dict ``render_features``
    returns -- of the frame seen through ``cam``; ``state``: what the previous step returned, with ``cam_prev`` the camera of that frame
    (both None: the first frame).  -> ``(out [H, W, 3], next_state)``; a state is a flat array of ``temporal_state_bytes`` bytes in the
    public layout of the header.  Keywords: ``make_temporal``.  Blocking; ``last_stats()`` is left as it was."""
    if isinstance(features, dict):
        features = features["raw"]
    image, features = np.asarray(image), np.asarray(features)
    T = image.dtype
    if T not in (np.dtype(np.float32), np.dtype(np.float64)) or features.dtype != T:
        raise TypeError("image and features must both be float32 or both float64")
    if image.ndim != 3 or image.shape[-1] != 3 or features.shape != image.shape[:-1] + (8,):
        raise ValueError(f"expected image [H, W, 3] and features [H, W, 8], got {image.shape} and {features.shape}")
    if 0 in image.shape:
        raise ValueError("empty image")
    if (state is None) != (cam_prev is None):
        raise ValueError("state and cam_prev must both be given or both be None (the first frame)")
    H, W = image.shape[:2]
    n_state = temporal_state_bytes(W, H, T) // T.itemsize
    Cm = _camera_arg(cam, T.type, "cam")
    Cp = None
    if state is not None:
        state = np.ascontiguousarray(state)
        if state.dtype != T or state.shape != (n_state,):
            raise ValueError(f"state must be a flat {T.name} array of {n_state} elements, got {state.dtype.name} {state.shape}")
        Cp = C.byref(_camera_arg(cam_prev, T.type, "cam_prev"))
    tp = make_temporal(**params)
    img = np.ascontiguousarray(np.swapaxes(image, 0, 1))             # the library's layout: pixel (i, j) at j*H + i
    feat = np.ascontiguousarray(np.swapaxes(features, 0, 1))
    out = np.empty((W, H, 3), dtype=T)
    nxt = np.zeros(n_state, dtype=T)
    fn = getattr(_capi.lib(), "rtw_temporal_" + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(C.byref(tp), C.byref(Cm), Cp, W, H, img.ctypes.data_as(C.c_void_p), feat.ctypes.data_as(C.c_void_p),
                   state.ctypes.data_as(C.c_void_p) if state is not None else None, nxt.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return np.swapaxes(out, 0, 1), nxt


def temporal_step_into(d_out_ptr, d_state_next_ptr, d_image_ptr, d_features_ptr, cam, image_width, image_height, *, d_state_prev_ptr=None, cam_prev=None,
                       elem_type=np.float32, stream=0, **params):
    """The device-resident form (rtw_temporal_device_*): enqueue one step on ``stream``.  All are DEVICE pointers: the linear image H*W*3
    elements, the features H*W*8 and both states of ``temporal_state_bytes`` bytes (16-byte aligned), the result H*W*3.  The result and the
    next state alias neither each other nor an input.  ``d_state_prev_ptr`` and ``cam_prev`` both None: the first frame.  Keywords:
    ``make_temporal``."""
    if (d_state_prev_ptr is None) != (cam_prev is None):
        raise ValueError("d_state_prev_ptr and cam_prev must both be given or both be None (the first frame)")
    T = np.dtype(elem_type).type
    Cm = _camera_arg(cam, T, "cam")
    Cp = C.byref(_camera_arg(cam_prev, T, "cam_prev")) if cam_prev is not None else None
    tp = make_temporal(**params)
    fn = getattr(_capi.lib(), "rtw_temporal_device_" + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(C.byref(tp), C.byref(Cm), Cp, int(image_width), int(image_height), C.c_void_p(int(d_image_ptr)), C.c_void_p(int(d_features_ptr)),
                   C.c_void_p(int(d_state_prev_ptr)) if d_state_prev_ptr is not None else None, C.c_void_p(int(d_state_next_ptr)), C.c_void_p(int(d_out_ptr)),
                   C.c_void_p(int(stream))))


class TemporalAccumulator:
    """The history of one camera path on one device: two device states (torch tensors; torch is the package's plumbing for device memory)
    and the previous frame's camera.  ``step`` enqueues one ``temporal_step_into`` and swaps the states; ``reset`` forgets the history, so
    the next step is a first frame.  Steps of one accumulator must be ordered on the device (one stream, or events between streams)."""

    def __init__(self, image_width, image_height, *, elem_type=np.float32, device=0, **params):
        import torch
        make_temporal(**params)                                    # (the keywords, checked now)
        self.width, self.height, self.elem_type = int(image_width), int(image_height), np.dtype(elem_type).type
        if self.width < 1 or self.height < 1:
            raise ValueError(f"empty frame {self.width} x {self.height}")
        self.params = dict(params, device=int(device))
        n = temporal_state_bytes(self.width, self.height, self.elem_type) // np.dtype(self.elem_type).itemsize
        dt = torch.float64 if _capi.is_f64(self.elem_type) else torch.float32
        self._states = [torch.zeros(n, dtype=dt, device=f"cuda:{int(device)}") for _ in range(2)]
        torch.cuda.synchronize(int(device))
        self._cur = 0                                              # the state the NEXT step writes
        self._cam_prev = None
        self.frames = 0

    @property
    def state(self):
        """the torch tensor that holds the state the last step left (None before the first step or after ``reset``)"""
        return self._states[self._cur ^ 1] if self._cam_prev is not None else None

    def reset(self):
        self._cam_prev = None
        self.frames = 0

    def step(self, cam, d_image_ptr, d_features_ptr, d_out_ptr, stream=0):
        if not isinstance(cam, Camera):
            raise TypeError("cam must be a Camera")
        prev = self._states[self._cur ^ 1].data_ptr() if self._cam_prev is not None else None
        temporal_step_into(d_out_ptr, self._states[self._cur].data_ptr(), d_image_ptr, d_features_ptr, cam, self.width, self.height, d_state_prev_ptr=prev,
                           cam_prev=self._cam_prev, elem_type=self.elem_type, stream=stream, **self.params)
        self._cur ^= 1
        self._cam_prev = cam
        self.frames += 1


def render_sequence(scene, cams, image_width=400, n_samples=1, *, seeds=None, denoise=None, depth=16, seed=1, n_chunks=0, device=-1, gamma=True, group_cull=False,
                    scan_valu=False, numerics=None, normal_power_log2=1, sigma_depth=0.1, min_weight=0.25, history_max=16.0, demodulate=True):
    """N cameras along a path over one scene with history reuse, in one call on the device (rtw_render_sequence_*): one batched render, one
    batched feature pass, ``len(cams)`` temporal steps in order (view 0 is a first frame) and, with ``denoise`` (True, or a dict of
    ``make_denoise``'s keywords ``levels, normal_power_log2, sigma_color, sigma_depth, demodulate``), one batched filter pass over the
    accumulated images.  ``gamma`` is applied once, by the last stage.  Returns ``img[v, i, j, :]``; ``last_stats()`` reports the render.
    ``seeds``: a sequence of ``len(cams)`` ints (None: ``seed`` for every view).  The temporal defaults are untuned (see the module's docstring)."""
    from .structs import flatten_scene
    cams, T = _batch_cameras(cams)
    n = len(cams)
    sd = _capi.make_seeds(seed if seeds is None else seeds, n)
    height = _frame_height(image_width, n_samples)
    D = None
    if denoise:
        dk = {} if denoise is True else dict(denoise)
        if set(dk) - set(_DENOISE_KEYS):
            raise ValueError(f"denoise takes the keywords {_DENOISE_KEYS}, got {sorted(set(dk) - set(_DENOISE_KEYS))}")
        D = make_denoise(gamma=gamma, **dk)
    tp = make_temporal(normal_power_log2, sigma_depth, min_weight, history_max, demodulate, gamma)
    L = _capi.lib()
    flat = scene if isinstance(scene, dict) else flatten_scene(scene, T)
    S, keep = _capi.make_scene(flat, T)
    P = _capi.make_params(image_width, height, n_samples, depth, seed, n_chunks, 0, 1, device, 1 if gamma else 0,
                          (_capi.FLAG_GROUP_CULL if group_cull else 0) | (_capi.FLAG_SCAN_VALU if scan_valu else 0), numerics=numerics)
    out = np.empty(n * height * int(image_width) * 3, dtype=T)
    fn = getattr(L, "rtw_render_sequence_" + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(C.byref(S), _capi.make_cameras(cams, T), n, sd, C.byref(P), C.byref(tp), C.byref(D) if D is not None else None, out.ctypes.data_as(C.c_void_p)))
    del keep
    _record_stats(L)
    return out.reshape(n, int(image_width), height, 3).transpose(0, 2, 1, 3)
