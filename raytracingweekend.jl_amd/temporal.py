"""Temporal reprojection (include/rtw_hip.h ``rtw_temporal_*``): history reuse along a camera path over one static scene.  A step blends
a frame's linear image with the history the previous frame left, gathered where the pixel's first-hit point lay in the previous view, under
weights from the feature buffers (coverage, normal, depth); the state (accumulated colour, guides, history length) travels from frame to
frame.  The definition is in the header; tests/temporal_ref.py restates it on the CPU and the device agrees on the bits.  All compute happens
in librtw_hip.so; there is no CPU fallback.

Defaults: ``normal_power_log2=1, sigma_depth=0.1, min_weight=0.25, history_max=16, demodulate=True, gamma=True``.  They are UNTUNED beyond a
small grid on the CPU witness.  The image handed to a step is a LINEAR one (``render(..., gamma=False)``): the step
applies gamma itself at the end, and the state stays linear.

Temporal moments (``rtw_history_moments_*``, ``rtw_history_noise_device_*``, ``rtw_render_path_guided_*``): the step can carry the
second moment of the luminance it accumulates in a plane of its own, and a second kernel turns state and moments into the per-pixel
relative-noise map the noise-guided filter takes -- a long history uses its own variance, a short one its neighbourhood's
(``temporal_step_moments``, ``temporal_step_moments_into``, ``temporal_noise_into``, ``TemporalAccumulator(moments=True)``,
``render_sequence(..., guided=True)``; witness: tests/temporal_noise_ref.py).  Its defaults ``radius=2, normal_power_log2=1,
sigma_depth=0.1, min_len=4`` are UNTUNED.

Temporal clamp (``rtw_clamped_step_*``, ``rtw_render_path_clamped_*``): the step can clamp the history it gathered to mean +- sigma
standard deviations of the current frame's window before it blends, and shorten the history it moved (``make_temporal_clamp``,
``temporal_step_clamped``, ``temporal_step_clamped_into``, ``TemporalAccumulator(clamp=...)``, ``render_sequence(..., clamp=...)``; witness:
tests/temporal_clamp_ref.py).  Its defaults ``radius=1, guides=False, sigma=1, len_scale=1`` are UNTUNED.  Omitting
``clamp`` is the plain step, call for call.

Batched steps (``rtw_reproject_*``, ``rtw_render_paths_*``): several independent camera paths over one scene (a stereo pair, orbiting
cameras) advance in EACH launch -- no new arithmetic, path s is the single call of path s on the bits; the per-path camera constants travel
in a device table (``temporal_path_table``, ``temporal_step_batch_into``, ``temporal_noise_batch_into``, ``TemporalBatchAccumulator``,
``render_sequences``; witness: tests/paths_ref.py, the single witnesses side by side; what it saves: DESIGN.md section 7.22).

Moving spheres (``rtw_motion_table_*``, ``rtw_first_hit_motion_*``, ``rtw_animated_step_*``): the steps above treat the world as static.  The
motion pass says per pixel which sphere its centre ray sees and how far that sphere moved since the previous frame (``motion_table``,
``first_hit_motion``, ``first_hit_motion_into``); the animated step subtracts that displacement from the pixel's world point before it
projects into the previous view (``temporal_step_animated``, ``temporal_step_animated_into``, ``TemporalAccumulator.step(...,
d_motion_ptr=...)``), and ``render_animation`` (``rtw_render_animation_*``) runs a list of scenes and cameras in one call.  With zero motion the step is
the static one on the bits.  Witness: tests/motion_ref.py; DESIGN.md section 7.23.
"""
import ctypes as C

import numpy as np

from . import _capi
from .denoise import GUIDED_SIGMA_COLOR, make_denoise
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


def _host_step(name, image, features, cam, state, moment, cam_prev, params, *, check, head=None, planes=True, moments=False, noise_map=False, motion=False):
    """One step on host arrays through the entry point ``name``: the checks of the arrays, then ``check()`` (the caller's own rule about its
    arguments; it raises), the state's and -- with ``moments`` -- the moment's, the library's layout,
    ``make_temporal(**params)`` and the struct ``head()`` makes behind it (``head`` returning None: a null pointer in its place), the call.
    ``planes``: the entry point takes the two moment planes (null without ``moments``); ``noise_map``: and the map.  ``motion`` other than
    False: rtw_animated_step_*'s argument order -- the motion plane [H, W, 4] (None on the first frame) behind the features, each moment
    plane behind its state.  -> ``(out [H, W, 3], next_state, next_moment or None, map [H, W] or None)``."""
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
    check()
    H, W = image.shape[:2]
    n_state = temporal_state_bytes(W, H, T) // T.itemsize
    n_mom = temporal_moment_bytes(W, H, T) // T.itemsize
    Cm = _camera_arg(cam, T.type, "cam")
    Cp = None
    if state is not None:
        state = np.ascontiguousarray(state)
        if state.dtype != T or state.shape != (n_state,):
            raise ValueError(f"state must be a flat {T.name} array of {n_state} elements, got {state.dtype.name} {state.shape}")
        if moments:
            moment = np.ascontiguousarray(moment)
            if moment.dtype != T or moment.shape != (n_mom,):
                raise ValueError(f"moment must be a flat {T.name} array of {n_mom} elements, got {moment.dtype.name} {moment.shape}")
        Cp = C.byref(_camera_arg(cam_prev, T.type, "cam_prev"))
    hd = head() if head else None
    heads = [C.byref(make_temporal(**params))] + ([C.byref(hd) if hd is not None else None] if head else [])
    img = np.ascontiguousarray(np.swapaxes(image, 0, 1))             # the library's layout: pixel (i, j) at j*H + i
    feat = np.ascontiguousarray(np.swapaxes(features, 0, 1))
    out, nxt = np.empty((W, H, 3), dtype=T), np.zeros(n_state, dtype=T)
    mom = np.zeros(n_mom, dtype=T) if moments else None
    rho = np.empty((W, H), dtype=T) if noise_map else None
    if motion is not False:
        mv = None
        if motion is not None:
            mv = np.asarray(motion)
            if mv.dtype != T or mv.shape != (H, W, 4):
                raise ValueError(f"motion must be a {T.name} array [H, W, 4] = {(H, W, 4)}, got {mv.dtype.name} {mv.shape}")
            mv = np.ascontiguousarray(np.swapaxes(mv, 0, 1))
        arrays = [img, feat, mv, state, nxt, moment if moments else None, mom, out]
    else:
        arrays = [img, feat, state] + ([moment if moments else None] if planes else []) + [nxt] + ([mom] if planes else []) + [out] + ([rho] if noise_map else [])
    fn = getattr(_capi.lib(), name + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(*heads, C.byref(Cm), Cp, W, H, *(a.ctypes.data_as(C.c_void_p) if a is not None else None for a in arrays)))
    return np.swapaxes(out, 0, 1), nxt, mom, np.swapaxes(rho, 0, 1) if noise_map else None


def _enqueue_step(name, cam, cam_prev, image_width, image_height, elem_type, stream, params, clamp, *ptrs, paths=None):
    """A device-resident step: the cameras, ``make_temporal(**params)``, with ``clamp`` its parameters behind them, the frame, the DEVICE
    pointers in the entry point's order (None: a null pointer) and the stream -> ``name`` + the element type's suffix.  ``paths``
    ``(n_paths, d_table_ptr)``: a batched step (rtw_reproject_batch_device_*) -- the count and the device table stand in the cameras' place
    and the clamp's slot is always there (None: plain steps)."""
    T = np.dtype(elem_type).type
    heads = [C.byref(make_temporal(**params))]
    if clamp is not None:
        heads.append(C.byref(make_temporal_clamp(**_clamp_arg(clamp))))
    if paths is not None:
        heads += ([None] if clamp is None else []) + [int(paths[0]), C.c_void_p(int(paths[1]))]
    else:
        Cm = _camera_arg(cam, T, "cam")
        heads += [C.byref(Cm), C.byref(_camera_arg(cam_prev, T, "cam_prev")) if cam_prev is not None else None]
    fn = getattr(_capi.lib(), name + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(*heads, int(image_width), int(image_height), *(C.c_void_p(int(q)) if q is not None else None for q in ptrs), C.c_void_p(int(stream))))


def temporal_step(image, features, cam, state=None, cam_prev=None, **params):
    """One step on host arrays (rtw_temporal_*): ``image`` [H, W, 3] (linear) and ``features`` [H, W, 8] -- or the dict ``render_features``
    returns -- of the frame seen through ``cam``; ``state``: what the previous step returned, with ``cam_prev`` the camera of that frame
    (both None: the first frame).  -> ``(out [H, W, 3], next_state)``; a state is a flat array of ``temporal_state_bytes`` bytes in the
    public layout of the header.  Keywords: ``make_temporal``.  Blocking; ``last_stats()`` is left as it was."""
    def check():
        if (state is None) != (cam_prev is None):
            raise ValueError("state and cam_prev must both be given or both be None (the first frame)")
    return _host_step("rtw_temporal_", image, features, cam, state, None, cam_prev, params, check=check, planes=False)[:2]


def temporal_step_into(d_out_ptr, d_state_next_ptr, d_image_ptr, d_features_ptr, cam, image_width, image_height, *, d_state_prev_ptr=None, cam_prev=None,
                       elem_type=np.float32, stream=0, **params):
    """The device-resident form (rtw_temporal_device_*): enqueue one step on ``stream``.  All are DEVICE pointers: the linear image H*W*3
    elements, the features H*W*8 and both states of ``temporal_state_bytes`` bytes (16-byte aligned), the result H*W*3.  The result and the
    next state alias neither each other nor an input.  ``d_state_prev_ptr`` and ``cam_prev`` both None: the first frame.  Keywords:
    ``make_temporal``."""
    if (d_state_prev_ptr is None) != (cam_prev is None):
        raise ValueError("d_state_prev_ptr and cam_prev must both be given or both be None (the first frame)")
    _enqueue_step("rtw_temporal_device_", cam, cam_prev, image_width, image_height, elem_type, stream, params, None, int(d_image_ptr), int(d_features_ptr), d_state_prev_ptr,
                  int(d_state_next_ptr), int(d_out_ptr))


_NOISE_KEYS = ("radius", "normal_power_log2", "sigma_depth", "min_len")


def make_temporal_noise(radius=2, normal_power_log2=1, sigma_depth=0.1, min_len=4.0, device=-1):
    """-> the ``rtw_temporal_noise_t`` of these keywords: the window of the spatial estimate and the history length from which a pixel's own
    moments are used.  The defaults are untuned beyond the record of DESIGN.md section 7.19."""
    return _capi.TemporalNoise(int(radius), int(normal_power_log2), int(device), (C.c_int32 * 3)(0, 0, 0), float(sigma_depth), float(min_len))


def _noise_arg(noise):
    """None / True / a dict of ``make_temporal_noise``'s keywords -> the keywords"""
    nk = {} if noise is None or noise is True else dict(noise)
    if set(nk) - set(_NOISE_KEYS):
        raise ValueError(f"noise takes the keywords {_NOISE_KEYS}, got {sorted(set(nk) - set(_NOISE_KEYS))}")
    return nk


def temporal_moment_bytes(image_width, image_height, elem_type=np.float32):
    """bytes of one moment plane: W*H elements rounded up to 16 bytes"""
    n = _capi.lib().rtw_history_moment_bytes(int(image_width), int(image_height), np.dtype(elem_type).itemsize)
    if n < 0:
        _capi.check(int(n))
    return int(n)


def temporal_step_moments(image, features, cam, state=None, moment=None, cam_prev=None, *, noise=None, **params):
    """``temporal_step`` with second moments and the noise map of what it leaves (rtw_history_moments_*): ``state``, ``moment`` and
    ``cam_prev`` are what the previous call returned and its camera (all None: the first frame).  -> ``(out [H, W, 3], next_state,
    next_moment, noise_map [H, W])``; a moment plane is a flat array of ``temporal_moment_bytes`` bytes, pixel (i, j) at j*H + i; the map is
    the per-pixel relative noise ``denoise``'s guided form takes (NaN where the pixel is not valid).  ``noise``: a dict of
    ``make_temporal_noise``'s keywords ``radius, normal_power_log2, sigma_depth, min_len`` (the defaults are untuned); other keywords:
    ``make_temporal``.  Blocking; ``last_stats()`` is left as it was."""
    def check():
        if not ((state is None) == (cam_prev is None) == (moment is None)):
            raise ValueError("state, moment and cam_prev must all be given or all be None (the first frame)")
    return _host_step("rtw_history_moments_", image, features, cam, state, moment, cam_prev, params, check=check, head=lambda: make_temporal_noise(**_noise_arg(noise)),
                      moments=True, noise_map=True)


def temporal_step_moments_into(d_out_ptr, d_state_next_ptr, d_moment_next_ptr, d_image_ptr, d_features_ptr, cam, image_width, image_height, *, d_state_prev_ptr=None,
                               d_moment_prev_ptr=None, cam_prev=None, elem_type=np.float32, stream=0, **params):
    """The device-resident step with moments (rtw_history_moments_device_*): ``temporal_step_into`` with the two moment planes, DEVICE
    pointers to ``temporal_moment_bytes`` bytes (16-byte aligned).  ``d_state_prev_ptr``, ``d_moment_prev_ptr`` and ``cam_prev`` all None:
    the first frame.  Keywords: ``make_temporal``."""
    if not ((d_state_prev_ptr is None) == (cam_prev is None) == (d_moment_prev_ptr is None)):
        raise ValueError("d_state_prev_ptr, d_moment_prev_ptr and cam_prev must all be given or all be None (the first frame)")
    _enqueue_step("rtw_history_moments_device_", cam, cam_prev, image_width, image_height, elem_type, stream, params, None, d_image_ptr, d_features_ptr, d_state_prev_ptr,
                  d_moment_prev_ptr, d_state_next_ptr, d_moment_next_ptr, d_out_ptr)


def _enqueue_noise(name, n_paths, d_noise_ptr, d_state_ptr, d_moment_ptr, image_width, image_height, elem_type, stream, noise):
    """A device-resident noise map through ``name`` + the element type's suffix; ``n_paths`` not None: the batched entry point's count"""
    tn = make_temporal_noise(**noise)
    T = np.dtype(elem_type).type
    fn = getattr(_capi.lib(), name + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(C.byref(tn), int(image_width), int(image_height), *([int(n_paths)] if n_paths is not None else []), C.c_void_p(int(d_state_ptr)),
                   C.c_void_p(int(d_moment_ptr)), C.c_void_p(int(d_noise_ptr)), C.c_void_p(int(stream))))


def temporal_noise_into(d_noise_ptr, d_state_ptr, d_moment_ptr, image_width, image_height, *, elem_type=np.float32, stream=0, **noise):
    """The device-resident noise map (rtw_history_noise_device_*): enqueue the map of a state and its moment plane on ``stream``.  All are
    DEVICE pointers; the map is H*W elements, pixel (i, j) at j*H + i -- what ``guided_filter``'s device forms read.  Keywords:
    ``make_temporal_noise`` (the defaults are untuned)."""
    _enqueue_noise("rtw_history_noise_device_", None, d_noise_ptr, d_state_ptr, d_moment_ptr, image_width, image_height, elem_type, stream, noise)


_CLAMP_KEYS = ("radius", "guides", "sigma", "len_scale")


def make_temporal_clamp(radius=1, guides=False, sigma=1.0, len_scale=1.0):
    """-> the ``rtw_temporal_clamp_t`` of these keywords: the window of the current frame is ``(2*radius + 1)^2``, ``guides`` weights its taps
    by the frame's coverage, normal and depth (RTW_CLAMP_GUIDES), the bounds are mean -+ ``sigma`` standard deviations, and the gathered
    history length of a pixel the clamp moved is multiplied by ``len_scale``.  The defaults are untuned beyond the record of DESIGN.md
    section 7.21."""
    return _capi.TemporalClamp(int(radius), _capi.CLAMP_GUIDES if guides else 0, (C.c_int32 * 2)(0, 0), float(sigma), float(len_scale))


def _clamp_arg(clamp):
    """True / a dict of ``make_temporal_clamp``'s keywords -> the keywords"""
    ck = {} if clamp is True else dict(clamp)
    if set(ck) - set(_CLAMP_KEYS):
        raise ValueError(f"clamp takes the keywords {_CLAMP_KEYS}, got {sorted(set(ck) - set(_CLAMP_KEYS))}")
    return ck


def temporal_step_clamped(image, features, cam, state=None, moment=None, cam_prev=None, *, clamp=True, moments=None, **params):
    """``temporal_step`` with the history clamped to the current frame's neighbourhood (rtw_clamped_step_*).  ``clamp``: True, or a dict
    of ``make_temporal_clamp``'s keywords ``radius, guides, sigma, len_scale`` (the defaults are untuned).  ``moments`` (default: whether
    ``moment`` is given): carry the second moments as ``temporal_step_moments`` does; ``state``, ``cam_prev`` (and with moments ``moment``)
    are None together: the first frame, which is the plain step's.  -> ``(out [H, W, 3], next_state)`` or, with moments,
    ``(out, next_state, next_moment)``.  Other keywords: ``make_temporal``.  Blocking; ``last_stats()`` is left as it was."""
    if moments is None:
        moments = moment is not None
    def check():
        if not clamp:
            raise ValueError("temporal_step_clamped needs clamp=True or a dict (without a clamp: temporal_step, temporal_step_moments)")
        if (state is None) != (cam_prev is None) or (moment is not None and (not moments or state is None)) or (moments and state is not None and moment is None):
            raise ValueError("state, cam_prev and (with moments) moment must all be given or all be None (the first frame)")
    res = _host_step("rtw_clamped_step_", image, features, cam, state, moment, cam_prev, params, check=check, head=lambda: make_temporal_clamp(**_clamp_arg(clamp)),
                     moments=moments)
    return res[:3] if moments else res[:2]


def temporal_step_clamped_into(d_out_ptr, d_state_next_ptr, d_image_ptr, d_features_ptr, cam, image_width, image_height, *, clamp=True, d_state_prev_ptr=None,
                               d_moment_prev_ptr=None, d_moment_next_ptr=None, cam_prev=None, elem_type=np.float32, stream=0, **params):
    """The device-resident clamped step (rtw_clamped_step_device_*): ``temporal_step_into`` -- or, with ``d_moment_next_ptr``,
    ``temporal_step_moments_into`` -- with ``clamp`` (True, or a dict of ``make_temporal_clamp``'s keywords; the defaults are untuned).
    ``d_state_prev_ptr``, ``cam_prev`` (and with moments ``d_moment_prev_ptr``) all None: the first frame.  Other keywords: ``make_temporal``."""
    if not clamp:
        raise ValueError("temporal_step_clamped_into needs clamp=True or a dict")
    if (d_state_prev_ptr is None) != (cam_prev is None) or (d_moment_prev_ptr is not None and (d_moment_next_ptr is None or d_state_prev_ptr is None)) or \
            (d_moment_next_ptr is not None and d_state_prev_ptr is not None and d_moment_prev_ptr is None):
        raise ValueError("d_state_prev_ptr, cam_prev and (with moments) d_moment_prev_ptr must all be given or all be None (the first frame)")
    _enqueue_step("rtw_clamped_step_device_", cam, cam_prev, image_width, image_height, elem_type, stream, params, clamp, d_image_ptr, d_features_ptr, d_state_prev_ptr,
                  d_moment_prev_ptr, d_state_next_ptr, d_moment_next_ptr, d_out_ptr)


# ---- moving spheres: the motion table, the first-hit motion pass and the animated step (include/rtw_hip.h rtw_first_hit_motion_*) ----

def _flat_scene(scene, T):
    from .structs import flatten_scene
    return scene if isinstance(scene, dict) else flatten_scene(scene, T)


def motion_table(scene_prev, scene, elem_type=np.float32):
    """The motion table of a frame (rtw_motion_table_*, host code): -> an array ``(n, 4)`` of ``elem_type``, row k = ``(dx, dy, dz, 0)`` of
    sphere k of ``scene`` since ``scene_prev`` -- one subtraction per component; three NaNs for a sphere that is new (``k >= n_prev``) or
    whose radius changed, so that its pixels reset.  Scenes: HittableLists or the flat dicts of ``flatten_scene``, in the same order."""
    T = np.dtype(elem_type).type
    Sp, keep_p = _capi.make_scene(_flat_scene(scene_prev, T), T)
    Sc, keep_c = _capi.make_scene(_flat_scene(scene, T), T)
    table = np.zeros((int(Sc.n), 4), dtype=T)
    fn = getattr(_capi.lib(), "rtw_motion_table_" + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(C.byref(Sp), C.byref(Sc), table.ctypes.data_as(C.c_void_p)))
    del keep_p, keep_c
    return table


def _motion_params(image_width, image_height, device, numerics, group_cull, scan_valu):
    from .structs import image_height as _ih
    H = int(image_height) if image_height is not None else _ih(image_width)
    if int(image_width) < 1 or H < 1:
        raise ValueError(f"empty frame {image_width} x {H}")
    flags = (_capi.FLAG_GROUP_CULL if group_cull else 0) | (_capi.FLAG_SCAN_VALU if scan_valu else 0)
    # (spp, depth, seed and chunks are not read by the pass: the render's defaults keep the struct valid)
    return H, _capi.make_params(int(image_width), H, 1, 16, 1, 0, 0, 1, int(device), 1, flags, numerics=numerics)


def first_hit_motion(scene, cam, image_width=400, image_height=None, *, table=None, device=-1, numerics=None, group_cull=False, scan_valu=False):
    """The first-hit motion pass on host arrays (rtw_first_hit_motion_*): -> ``[H, W, 4]``, per pixel ``(m.x, m.y, m.z, id)`` -- the row of
    ``table`` (``motion_table``; None: zeros, an id / picking buffer) of the sphere the pixel's centre ray sees first, and that sphere's
    index in the scene's order as a float (-1: the sky).  The ray is the temporal step's own (no lens, no jitter); among equal hits the
    lower index wins.  ``image_height`` None: the package's 16:9 height.  ``group_cull`` / ``scan_valu`` are accepted and change nothing.
    Blocking; ``last_stats()`` is left as it was."""
    if not isinstance(cam, Camera):
        raise TypeError("cam must be a Camera")
    T = np.dtype(cam.elem_type).type
    H, P = _motion_params(image_width, image_height, device, numerics, group_cull, scan_valu)
    S, keep = _capi.make_scene(_flat_scene(scene, T), T)
    tab = None
    if table is not None:
        tab = np.ascontiguousarray(table)
        if tab.dtype != T or tab.shape != (int(S.n), 4):
            raise ValueError(f"table must be a {np.dtype(T).name} array {(int(S.n), 4)}, got {tab.dtype.name} {tab.shape}")
    out = np.empty((int(image_width), H, 4), dtype=T)
    fn = getattr(_capi.lib(), "rtw_first_hit_motion_" + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(C.byref(S), C.byref(_capi.make_camera(cam, T)), C.byref(P), tab.ctypes.data_as(C.c_void_p) if tab is not None else None, out.ctypes.data_as(C.c_void_p)))
    del keep
    return np.swapaxes(out, 0, 1)


def first_hit_motion_into(renderer, d_motion_ptr, image_width, image_height=None, *, cam=None, d_table_ptr=None, stream=0, numerics=None, group_cull=False,
                          scan_valu=False):
    """The device-resident form (rtw_first_hit_motion_device_*): enqueue the pass of ``renderer``'s scene (a ``DeviceRenderer``) through
    ``cam`` (None: the renderer's camera) on ``stream``.  ``d_motion_ptr``: H*W*4 elements, pixel (i, j) at slot ``j*H + i``;
    ``d_table_ptr``: the uploaded ``motion_table`` (None: m = 0); both DEVICE pointers, 16-byte aligned.  Returns H."""
    T = np.dtype(renderer.T).type
    H, P = _motion_params(image_width, image_height, -1, numerics, group_cull, scan_valu)
    Cm = renderer.cam if cam is None else _camera_arg(cam, T, "cam")
    fn = getattr(renderer.L, "rtw_first_hit_motion_device_" + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(renderer.handle, C.byref(Cm), C.byref(P), C.c_void_p(int(d_table_ptr)) if d_table_ptr is not None else None, C.c_void_p(int(d_motion_ptr)),
                   C.c_void_p(int(stream))))
    return H


def temporal_step_animated(image, features, cam, motion=None, state=None, moment=None, cam_prev=None, *, clamp=None, moments=None, **params):
    """One step over a moving scene on host arrays (rtw_animated_step_*): ``temporal_step`` -- with ``moments`` the step with moments, with
    ``clamp`` (True, or a dict of ``make_temporal_clamp``'s keywords) the clamped one -- whose world points are moved back by ``motion``, the
    ``[H, W, 4]`` plane of ``first_hit_motion`` for this frame.  ``motion``, ``state``, ``cam_prev`` (and with moments ``moment``) are None
    together: the first frame.  -> ``(out [H, W, 3], next_state)`` or, with moments, ``(out, next_state, next_moment)``.  With a plane of
    zeros the result is the static step's on the bits.  Other keywords: ``make_temporal``.  Blocking."""
    if moments is None:
        moments = moment is not None
    def check():
        if not ((state is None) == (cam_prev is None) == (motion is None)) or (moment is not None and (not moments or state is None)) or \
                (moments and state is not None and moment is None):
            raise ValueError("motion, state, cam_prev and (with moments) moment must all be given or all be None (the first frame)")
    res = _host_step("rtw_animated_step_", image, features, cam, state, moment, cam_prev, params, check=check,
                     head=lambda: make_temporal_clamp(**_clamp_arg(clamp)) if clamp else None, moments=moments, motion=motion)
    return res[:3] if moments else res[:2]


def temporal_step_animated_into(d_out_ptr, d_state_next_ptr, d_image_ptr, d_features_ptr, cam, image_width, image_height, *, d_motion_ptr=None, clamp=None,
                                d_state_prev_ptr=None, d_moment_prev_ptr=None, d_moment_next_ptr=None, cam_prev=None, elem_type=np.float32, stream=0, **params):
    """The device-resident step over a moving scene (rtw_animated_step_device_*): ``temporal_step_into`` / ``temporal_step_moments_into`` /
    ``temporal_step_clamped_into`` (by ``clamp`` and the moment pointers) with the motion plane ``d_motion_ptr`` -- H*W*4 elements, 16-byte
    aligned, what ``first_hit_motion_into`` wrote for this frame.  ``d_motion_ptr``, ``d_state_prev_ptr``, ``cam_prev`` (and with moments
    ``d_moment_prev_ptr``) all None: the first frame.  One launch.  Other keywords: ``make_temporal``."""
    if not ((d_state_prev_ptr is None) == (cam_prev is None) == (d_motion_ptr is None)) or (d_moment_prev_ptr is not None and (d_moment_next_ptr is None or d_state_prev_ptr is None)) or \
            (d_moment_next_ptr is not None and d_state_prev_ptr is not None and d_moment_prev_ptr is None):
        raise ValueError("d_motion_ptr, d_state_prev_ptr, cam_prev and (with moments) d_moment_prev_ptr must all be given or all be None (the first frame)")
    T = np.dtype(elem_type).type
    K = make_temporal_clamp(**_clamp_arg(clamp)) if clamp else None
    Cm = _camera_arg(cam, T, "cam")
    ptrs = (d_image_ptr, d_features_ptr, d_motion_ptr, d_state_prev_ptr, d_state_next_ptr, d_moment_prev_ptr, d_moment_next_ptr, d_out_ptr)
    fn = getattr(_capi.lib(), "rtw_animated_step_device_" + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(C.byref(make_temporal(**params)), C.byref(K) if K is not None else None, C.byref(Cm),
                   C.byref(_camera_arg(cam_prev, T, "cam_prev")) if cam_prev is not None else None, int(image_width), int(image_height),
                   *(C.c_void_p(int(q)) if q is not None else None for q in ptrs), C.c_void_p(int(stream))))


def render_animation(scenes, cams, image_width=400, n_samples=1, *, seeds=None, denoise=None, clamp=None, blur=None, depth=16, seed=1, n_chunks=0, device=-1, gamma=True,
                     group_cull=False, scan_valu=False, numerics=None, **params):
    """``len(scenes)`` frames of a scene whose spheres move (and a camera that may), with history reuse across the motion, in one call on
    the device (rtw_render_animation_*): per frame the scene's upload, a linear render, its feature pass, from frame 1 on the motion table
    against the previous frame's scene and the motion pass, then the step (frame 0 is a first frame); with ``denoise`` (True, or a dict of
    ``make_denoise``'s keywords ``levels, normal_power_log2, sigma_color, sigma_depth, demodulate``) one batched filter pass over the
    accumulated frames; one copy back.  Frame v equals the chain of ``render``, ``render_features``, ``motion_table``, ``first_hit_motion``
    and ``temporal_step_animated`` (and ``denoise_batch``) on the bits.  ``scenes``: HittableLists (or flat dicts) with the spheres in the
    same order; ``cams``: as many cameras; ``seeds``: as many ints (None: ``seed``).  ``clamp``: as ``render_sequence``; other keywords:
    ``make_temporal``'s.  ``gamma`` is applied once, by the last stage.  Returns ``img[v, i, j, :]``; ``last_stats()`` sums the renders.
    ``blur`` (True, or a dict of ``make_motion_blur``'s keywords ``taps, shutter, depth_extent``): the motion-blur stage behind the last linear
    stage of every frame from 1 on (rtw_render_blurred_*; frame 0 has no previous camera and passes through) -- frame v is then
    ``motion_blur`` of frame v of the same call with ``gamma=False``, on the bits."""
    scenes = list(scenes)
    cams, T = _batch_cameras(cams)
    n = len(cams)
    if len(scenes) != n:
        raise ValueError(f"{len(scenes)} scenes for {n} cameras")
    sd = _capi.make_seeds(seed if seeds is None else seeds, n)
    height = _frame_height(image_width, n_samples)
    D = None
    if denoise:
        dk = {} if denoise is True else dict(denoise)
        if set(dk) - set(_DENOISE_KEYS):
            raise ValueError(f"denoise takes the keywords {_DENOISE_KEYS}, got {sorted(set(dk) - set(_DENOISE_KEYS))}")
        D = make_denoise(gamma=gamma, **dk)
    tp = make_temporal(gamma=gamma, **params)
    K = make_temporal_clamp(**_clamp_arg(clamp)) if clamp else None
    made = [_capi.make_scene(_flat_scene(s, T), T) for s in scenes]
    S = (type(made[0][0]) * n)(*[m[0] for m in made])
    P = _capi.make_params(image_width, height, n_samples, depth, seed, n_chunks, 0, 1, device, 1 if gamma else 0,
                          (_capi.FLAG_GROUP_CULL if group_cull else 0) | (_capi.FLAG_SCAN_VALU if scan_valu else 0), numerics=numerics)
    out = np.empty(n * height * int(image_width) * 3, dtype=T)
    L = _capi.lib()
    tail = []
    if blur:
        from .motion_blur import _BLUR_KEYS, make_motion_blur
        bk = {} if blur is True else dict(blur)
        if set(bk) - set(_BLUR_KEYS):
            raise ValueError(f"blur takes the keywords {_BLUR_KEYS}, got {sorted(set(bk) - set(_BLUR_KEYS))}")
        B = make_motion_blur(gamma=gamma, **bk)
        tail = [C.byref(B)]
    fn = getattr(L, ("rtw_render_blurred_" if blur else "rtw_render_animation_") + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(S, _capi.make_cameras(cams, T), n, sd, C.byref(P), C.byref(tp), C.byref(K) if K is not None else None, C.byref(D) if D is not None else None,
                   *tail, out.ctypes.data_as(C.c_void_p)))
    del made
    _record_stats(L)
    return out.reshape(n, int(image_width), height, 3).transpose(0, 2, 1, 3)


class TemporalAccumulator:
    """The history of one camera path on one device: two device states (torch tensors; torch is the package's plumbing for device memory)
    and the previous frame's camera.  ``step`` enqueues one ``temporal_step_into`` and swaps the states; ``reset`` forgets the history, so
    the next step is a first frame.  Steps of one accumulator must be ordered on the device (one stream, or events between streams).
    ``moments=True``: the steps carry second moments (``temporal_step_moments_into``, two moment planes besides the states) and
    ``noise_into`` enqueues the noise map of the state the last step left.  ``clamp`` (True, or a dict of ``make_temporal_clamp``'s keywords):
    every step is a clamped step (``temporal_step_clamped_into``), with or without moments; None: the plain steps, call for call."""

    def __init__(self, image_width, image_height, *, elem_type=np.float32, device=0, moments=False, clamp=None, **params):
        import torch
        make_temporal(**params)                                    # (the keywords, checked now)
        self.clamp = _clamp_arg(clamp) if clamp else None
        if self.clamp is not None:
            make_temporal_clamp(**self.clamp)
        self.width, self.height, self.elem_type = int(image_width), int(image_height), np.dtype(elem_type).type
        if self.width < 1 or self.height < 1:
            raise ValueError(f"empty frame {self.width} x {self.height}")
        self.params = dict(params, device=int(device))
        self.moments = bool(moments)
        n = temporal_state_bytes(self.width, self.height, self.elem_type) // np.dtype(self.elem_type).itemsize
        dt = torch.float64 if _capi.is_f64(self.elem_type) else torch.float32
        self._states = [torch.zeros(n, dtype=dt, device=f"cuda:{int(device)}") for _ in range(2)]
        self._moments = None
        if self.moments:
            nm = temporal_moment_bytes(self.width, self.height, self.elem_type) // np.dtype(self.elem_type).itemsize
            self._moments = [torch.zeros(nm, dtype=dt, device=f"cuda:{int(device)}") for _ in range(2)]
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

    def step(self, cam, d_image_ptr, d_features_ptr, d_out_ptr, stream=0, d_motion_ptr=None):
        """``d_motion_ptr``: the motion plane of this frame (``first_hit_motion_into``) -- the step over a moving scene
        (``temporal_step_animated_into``); it is ignored on a first frame, which has no history to move.  None: the static steps, call for call."""
        if not isinstance(cam, Camera):
            raise TypeError("cam must be a Camera")
        prev = self._states[self._cur ^ 1].data_ptr() if self._cam_prev is not None else None
        if d_motion_ptr is not None:
            mprev = self._moments[self._cur ^ 1].data_ptr() if self.moments and self._cam_prev is not None else None
            temporal_step_animated_into(d_out_ptr, self._states[self._cur].data_ptr(), d_image_ptr, d_features_ptr, cam, self.width, self.height,
                                        d_motion_ptr=d_motion_ptr if prev is not None else None, clamp=self.clamp, d_state_prev_ptr=prev, d_moment_prev_ptr=mprev,
                                        d_moment_next_ptr=self._moments[self._cur].data_ptr() if self.moments else None, cam_prev=self._cam_prev,
                                        elem_type=self.elem_type, stream=stream, **self.params)
        elif self.clamp is not None:
            mprev = self._moments[self._cur ^ 1].data_ptr() if self.moments and self._cam_prev is not None else None
            temporal_step_clamped_into(d_out_ptr, self._states[self._cur].data_ptr(), d_image_ptr, d_features_ptr, cam, self.width, self.height, clamp=self.clamp,
                                       d_state_prev_ptr=prev, d_moment_prev_ptr=mprev, d_moment_next_ptr=self._moments[self._cur].data_ptr() if self.moments else None,
                                       cam_prev=self._cam_prev, elem_type=self.elem_type, stream=stream, **self.params)
        elif self.moments:
            mprev = self._moments[self._cur ^ 1].data_ptr() if self._cam_prev is not None else None
            temporal_step_moments_into(d_out_ptr, self._states[self._cur].data_ptr(), self._moments[self._cur].data_ptr(), d_image_ptr, d_features_ptr, cam, self.width,
                                       self.height, d_state_prev_ptr=prev, d_moment_prev_ptr=mprev, cam_prev=self._cam_prev, elem_type=self.elem_type, stream=stream, **self.params)
        else:
            temporal_step_into(d_out_ptr, self._states[self._cur].data_ptr(), d_image_ptr, d_features_ptr, cam, self.width, self.height, d_state_prev_ptr=prev,
                               cam_prev=self._cam_prev, elem_type=self.elem_type, stream=stream, **self.params)
        self._cur ^= 1
        self._cam_prev = cam
        self.frames += 1

    @property
    def moment(self):
        """the torch tensor that holds the moment plane the last step left (None without ``moments=True``, before the first step or after ``reset``)"""
        return self._moments[self._cur ^ 1] if self.moments and self._cam_prev is not None else None

    def noise_into(self, d_noise_ptr, stream=0, **noise):
        """enqueue the noise map (``temporal_noise_into``) of the state and moments the last step left; keywords: ``make_temporal_noise``"""
        if not self.moments:
            raise ValueError("noise_into needs an accumulator made with moments=True")
        if self._cam_prev is None:
            raise ValueError("noise_into before the first step: there is no state yet")
        temporal_noise_into(d_noise_ptr, self.state.data_ptr(), self.moment.data_ptr(), self.width, self.height, elem_type=self.elem_type, stream=stream,
                            device=self.params["device"], **noise)


def render_sequence(scene, cams, image_width=400, n_samples=1, *, seeds=None, denoise=None, guided=None, clamp=None, depth=16, seed=1, n_chunks=0, device=-1, gamma=True,
                    group_cull=False, scan_valu=False, numerics=None, normal_power_log2=1, sigma_depth=0.1, min_weight=0.25, history_max=16.0, demodulate=True):
    """N cameras along a path over one scene with history reuse, in one call on the device (rtw_render_sequence_*): one batched render, one
    batched feature pass, ``len(cams)`` temporal steps in order (view 0 is a first frame) and, with ``denoise`` (True, or a dict of
    ``make_denoise``'s keywords ``levels, normal_power_log2, sigma_color, sigma_depth, demodulate``), one batched filter pass over the
    accumulated images.  ``guided`` (True, or a dict of ``make_temporal_noise``'s keywords ``radius, normal_power_log2, sigma_depth,
    min_len``; rtw_render_path_guided_*): the steps carry second moments, a noise map follows each step and the filter pass is the
    noise-guided one over those maps -- ``denoise`` is then required (None: its defaults, ``sigma_color`` defaults to ``GUIDED_SIGMA_COLOR``) and its
    ``demodulate`` must be the steps'.  ``clamp`` (True, or a dict of ``make_temporal_clamp``'s keywords ``radius, guides, sigma, len_scale``;
    rtw_render_path_clamped_*): the steps behind view 0 are clamped steps, in any of the three forms above; the clamp's defaults are untuned.
    ``gamma`` is applied once, by the last stage.  Returns ``img[v, i, j, :]``; ``last_stats()`` reports the render.
    ``seeds``: a sequence of ``len(cams)`` ints (None: ``seed`` for every view).  The temporal defaults are untuned (see the module's docstring)."""
    return _render_frames(scene, cams, 0, image_width, n_samples, seeds=seeds, denoise=denoise, guided=guided, clamp=clamp, depth=depth, seed=seed, n_chunks=n_chunks,
                          device=device, gamma=gamma, group_cull=group_cull, scan_valu=scan_valu, numerics=numerics, normal_power_log2=normal_power_log2,
                          sigma_depth=sigma_depth, min_weight=min_weight, history_max=history_max, demodulate=demodulate)


def _render_frames(scene, cams, n_paths, image_width, n_samples, *, seeds=None, denoise=None, guided=None, clamp=None, depth=16, seed=1, n_chunks=0, device=-1, gamma=True,
                   group_cull=False, scan_valu=False, numerics=None, normal_power_log2=1, sigma_depth=0.1, min_weight=0.25, history_max=16.0, demodulate=True):
    """The one marshalling of the sequence calls.  ``n_paths == 0``: ``render_sequence``'s entry points over the path ``cams``; ``n_paths >= 1``:
    rtw_render_paths_* over ``cams`` and ``seeds`` in STEP-major order (path s at step k: entry ``k*n_paths + s``).  -> ``img[frame, i, j, :]``"""
    from .structs import flatten_scene
    cams, T = _batch_cameras(cams)
    n = len(cams)
    sd = _capi.make_seeds(seed if seeds is None else seeds, n)
    height = _frame_height(image_width, n_samples)
    D = N = None
    if guided:
        N = make_temporal_noise(**_noise_arg(guided))
        if denoise is None:
            denoise = True
        elif not denoise:
            raise ValueError("guided=... filters with the noise map: denoise may not be switched off")
    if denoise:
        dk = {} if denoise is True else dict(denoise)
        if set(dk) - set(_DENOISE_KEYS):
            raise ValueError(f"denoise takes the keywords {_DENOISE_KEYS}, got {sorted(set(dk) - set(_DENOISE_KEYS))}")
        if guided:
            dk.setdefault("sigma_color", GUIDED_SIGMA_COLOR)       # (there it counts estimated standard deviations: denoise.py)
        D = make_denoise(gamma=gamma, **dk)
        if guided and bool(dk.get("demodulate", True)) != bool(demodulate):
            raise ValueError("guided=...: denoise's demodulate must equal the steps' (the noise map is relative to the state's luminance)")
    tp = make_temporal(normal_power_log2, sigma_depth, min_weight, history_max, demodulate, gamma)
    L = _capi.lib()
    flat = scene if isinstance(scene, dict) else flatten_scene(scene, T)
    S, keep = _capi.make_scene(flat, T)
    P = _capi.make_params(image_width, height, n_samples, depth, seed, n_chunks, 0, 1, device, 1 if gamma else 0,
                          (_capi.FLAG_GROUP_CULL if group_cull else 0) | (_capi.FLAG_SCAN_VALU if scan_valu else 0), numerics=numerics)
    out = np.empty(n * height * int(image_width) * 3, dtype=T)
    sfx = "f64" if _capi.is_f64(T) else "f32"
    if n_paths:
        K = make_temporal_clamp(**_clamp_arg(clamp)) if clamp else None
        _capi.check(getattr(L, "rtw_render_paths_" + sfx)(C.byref(S), _capi.make_cameras(cams, T), int(n_paths), n // int(n_paths), sd, C.byref(P), C.byref(tp),
                                                          C.byref(K) if K is not None else None, C.byref(N) if N is not None else None,
                                                          C.byref(D) if D is not None else None, out.ctypes.data_as(C.c_void_p)))
    elif clamp:
        K = make_temporal_clamp(**_clamp_arg(clamp))
        _capi.check(getattr(L, "rtw_render_path_clamped_" + sfx)(C.byref(S), _capi.make_cameras(cams, T), n, sd, C.byref(P), C.byref(tp), C.byref(K),
                                                                 C.byref(N) if N is not None else None, C.byref(D) if D is not None else None,
                                                                 out.ctypes.data_as(C.c_void_p)))
    elif N is not None:
        _capi.check(getattr(L, "rtw_render_path_guided_" + sfx)(C.byref(S), _capi.make_cameras(cams, T), n, sd, C.byref(P), C.byref(tp), C.byref(N), C.byref(D),
                                                                    out.ctypes.data_as(C.c_void_p)))
    else:
        _capi.check(getattr(L, "rtw_render_sequence_" + sfx)(C.byref(S), _capi.make_cameras(cams, T), n, sd, C.byref(P), C.byref(tp), C.byref(D) if D is not None else None,
                                                             out.ctypes.data_as(C.c_void_p)))
    del keep
    _record_stats(L)
    return out.reshape(n, int(image_width), height, 3).transpose(0, 2, 1, 3)


# ---- batched steps: n_paths independent camera paths advance in each launch (include/rtw_hip.h rtw_reproject_*, rtw_render_paths_*) ----

def temporal_path_table(cams, cams_prev=None, elem_type=None):
    """The camera constants of ``len(cams)`` paths (rtw_reproject_table_*): -> a host array ``(n_paths, 32)`` in the header's public layout --
    the current camera's origin, lower_left_corner, horizontal, vertical; the previous camera's origin, w, horizontal, vertical; Kw, Qh, Qv,
    ih, iv; three zeros.  ``cams_prev`` None (first frames): elements 12..28 are 0.  ``elem_type``: None takes the cameras'.  The caller
    uploads it; a batched step reads it on the device."""
    cams, T = _batch_cameras(cams)
    if elem_type is not None:
        T = np.dtype(elem_type).type
    n = len(cams)
    Cp = None
    if cams_prev is not None:
        cams_prev = list(cams_prev)
        if len(cams_prev) != n:
            raise ValueError(f"{len(cams_prev)} previous cameras for {n} paths")
        for c in cams_prev:
            _camera_arg(c, T, "cams_prev")                          # (the type and the element type, checked)
        Cp = _capi.make_cameras(cams_prev, T)
    for c in cams:
        _camera_arg(c, T, "cams")
    table = np.zeros((n, 32), dtype=T)
    fn = getattr(_capi.lib(), "rtw_reproject_table_" + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(_capi.make_cameras(cams, T), Cp, n, table.ctypes.data_as(C.c_void_p)))
    return table


def temporal_step_batch_into(d_out_ptr, d_states_next_ptr, d_images_ptr, d_features_ptr, d_table_ptr, n_paths, image_width, image_height, *, clamp=None,
                             d_states_prev_ptr=None, d_moments_prev_ptr=None, d_moments_next_ptr=None, elem_type=np.float32, stream=0, **params):
    """The device-resident batched step (rtw_reproject_batch_device_*): ``n_paths`` paths advance in ONE launch on ``stream``; path s is, on the
    bits, ``temporal_step_into`` / ``temporal_step_moments_into`` / ``temporal_step_clamped_into`` of path s.  All are DEVICE pointers; every
    buffer holds the paths one behind the other (states at ``temporal_state_bytes``, moment planes at ``temporal_moment_bytes``);
    ``d_table_ptr``: the uploaded ``temporal_path_table``.  ``clamp`` None: plain steps; no moment pointer: no moments;
    ``d_states_prev_ptr`` None: every path's first frame.  Other keywords: ``make_temporal``."""
    _enqueue_step("rtw_reproject_batch_device_", None, None, image_width, image_height, elem_type, stream, params, clamp if clamp else None, d_images_ptr, d_features_ptr,
                  d_states_prev_ptr, d_moments_prev_ptr, d_states_next_ptr, d_moments_next_ptr, d_out_ptr, paths=(n_paths, d_table_ptr))


def temporal_noise_batch_into(d_noise_ptr, d_states_ptr, d_moments_ptr, n_paths, image_width, image_height, *, elem_type=np.float32, stream=0, **noise):
    """The device-resident batched noise map (rtw_reproject_noise_batch_device_*): the maps of ``n_paths`` states and their moment planes, one
    behind the other (``n_paths * H * W`` elements), in ONE launch on ``stream``.  Keywords: ``make_temporal_noise``."""
    _enqueue_noise("rtw_reproject_noise_batch_device_", n_paths, d_noise_ptr, d_states_ptr, d_moments_ptr, image_width, image_height, elem_type, stream, noise)


class TemporalBatchAccumulator:
    """The histories of ``n_paths`` camera paths of one frame size on one device: two SETS of device states (with ``moments=True`` of moment
    planes too), the device table of the paths' camera constants and the previous step's cameras.  ``step`` uploads the table on ``stream``
    (ordered before the launch), enqueues ONE ``temporal_step_batch_into`` for all paths and swaps the sets; ``reset`` forgets every history.
    All paths step together: there is no path that joins or resets alone.  ``clamp`` / ``moments`` / keywords: as ``TemporalAccumulator``."""

    def __init__(self, n_paths, image_width, image_height, *, elem_type=np.float32, device=0, moments=False, clamp=None, **params):
        import torch
        make_temporal(**params)                                    # (the keywords, checked now)
        self.clamp = _clamp_arg(clamp) if clamp else None
        if self.clamp is not None:
            make_temporal_clamp(**self.clamp)
        self.n_paths, self.width, self.height, self.elem_type = int(n_paths), int(image_width), int(image_height), np.dtype(elem_type).type
        if self.n_paths < 1:
            raise ValueError(f"n_paths must be >= 1, got {self.n_paths}")
        if self.width < 1 or self.height < 1:
            raise ValueError(f"empty frame {self.width} x {self.height}")
        self.params = dict(params, device=int(device))
        self.moments = bool(moments)
        item = np.dtype(self.elem_type).itemsize
        self._n_state = temporal_state_bytes(self.width, self.height, self.elem_type) // item
        self._n_mom = temporal_moment_bytes(self.width, self.height, self.elem_type) // item
        dt = torch.float64 if _capi.is_f64(self.elem_type) else torch.float32
        dev = f"cuda:{int(device)}"
        self._states = [torch.zeros(self.n_paths * self._n_state, dtype=dt, device=dev) for _ in range(2)]
        self._moments = [torch.zeros(self.n_paths * self._n_mom, dtype=dt, device=dev) for _ in range(2)] if self.moments else None
        self._table = torch.zeros(self.n_paths * 32, dtype=dt, device=dev)
        torch.cuda.synchronize(int(device))
        self._cur = 0                                              # the set the NEXT step writes
        self._cams_prev = None
        self.frames = 0

    def reset(self):
        self._cams_prev = None
        self.frames = 0

    def state(self, s):
        """the torch tensor (a view) that holds the state the last step left for path ``s`` (None before the first step or after ``reset``)"""
        if self._cams_prev is None:
            return None
        return self._states[self._cur ^ 1][int(s) * self._n_state:(int(s) + 1) * self._n_state]

    def moment(self, s):
        """... and its moment plane (None without ``moments=True``)"""
        if self._cams_prev is None or not self.moments:
            return None
        return self._moments[self._cur ^ 1][int(s) * self._n_mom:(int(s) + 1) * self._n_mom]

    def step(self, cams, d_images_ptr, d_features_ptr, d_out_ptr, stream=0):
        import torch
        cams = list(cams)
        if len(cams) != self.n_paths:
            raise ValueError(f"{len(cams)} cameras for {self.n_paths} paths")
        table = torch.from_numpy(temporal_path_table(cams, self._cams_prev, self.elem_type).reshape(-1))
        # (from pageable memory: the copy has left the host array when copy_ returns, and runs on `stream` in front of the launch)
        with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=self._table.device) if int(stream) else torch.cuda.default_stream(self._table.device)):
            self._table.copy_(table, non_blocking=True)
        first = self._cams_prev is None
        temporal_step_batch_into(d_out_ptr, self._states[self._cur].data_ptr(), d_images_ptr, d_features_ptr, self._table.data_ptr(), self.n_paths, self.width, self.height,
                                 clamp=self.clamp, d_states_prev_ptr=None if first else self._states[self._cur ^ 1].data_ptr(),
                                 d_moments_prev_ptr=None if first or not self.moments else self._moments[self._cur ^ 1].data_ptr(),
                                 d_moments_next_ptr=self._moments[self._cur].data_ptr() if self.moments else None, elem_type=self.elem_type, stream=stream, **self.params)
        self._cur ^= 1
        self._cams_prev = cams
        self.frames += 1

    def noise_into(self, d_noise_ptr, stream=0, **noise):
        """enqueue the ``n_paths`` noise maps (``temporal_noise_batch_into``) of the states and moments the last step left"""
        if not self.moments:
            raise ValueError("noise_into needs an accumulator made with moments=True")
        if self._cams_prev is None:
            raise ValueError("noise_into before the first step: there is no state yet")
        temporal_noise_batch_into(d_noise_ptr, self._states[self._cur ^ 1].data_ptr(), self._moments[self._cur ^ 1].data_ptr(), self.n_paths, self.width, self.height,
                                  elem_type=self.elem_type, stream=stream, device=self.params["device"], **noise)


def render_sequences(scene, paths, image_width=400, n_samples=1, *, seeds=None, **kw):
    """``S = len(paths)`` camera paths of equal length N over one scene, each with its own history, in ONE call on the device
    (rtw_render_paths_*): one batched render and one feature pass over all S*N views, N batched step launches (every launch advances all
    S paths), with ``guided`` N batched noise launches, with ``denoise`` one batched filter pass.  ``paths``: a list of S equally long lists
    of cameras; ``seeds``: None (``seed`` for every view) or S sequences of N ints.  Everything else: ``render_sequence``'s keywords, and
    path s of the result equals ``render_sequence(scene, paths[s], ..., seeds=seeds[s])`` on the bits.  Returns ``img[s, k, i, j, :]``
    (path, step).  The transposition to the library's step-major order happens here and nowhere else."""
    paths = [list(p) for p in paths]
    if not paths or not paths[0] or any(len(p) != len(paths[0]) for p in paths):
        raise ValueError("paths must be a non-empty list of equally long, non-empty camera lists")
    S, N = len(paths), len(paths[0])
    if seeds is not None:
        seeds = [list(sd) for sd in seeds]
        if len(seeds) != S or any(len(sd) != N for sd in seeds):
            raise ValueError(f"seeds must be {S} sequences of {N} ints")
        seeds = [seeds[s][k] for k in range(N) for s in range(S)]
    out = _render_frames(scene, [paths[s][k] for k in range(N) for s in range(S)], S, image_width, n_samples, seeds=seeds, **kw)
    return out.reshape((N, S) + out.shape[1:]).swapaxes(0, 1)
