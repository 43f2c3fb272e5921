"""Radiance queries (include/rtw_hip.h ``rtw_trace_rays_*``): ``ray_color`` along caller-supplied rays -- the Monte Carlo estimate the
renders are built around on rays that belong to no pixel and no camera: light and irradiance probes, light baking at surface points,
reflection captures, the rays of a camera model of the caller's own, the continuation of paths a caller started itself.

The rays are those of ``rays.cast_rays`` (8 elements ``ox oy oz dx dy dz tmax tag``; the last two are not read).  Sample ``s`` of ray ``i``
is the reference's ``ray_color(scene, o_i, d_i, max_depth)`` on the fresh stream ``(seed, first_stream + i, first_sample + s)``; the result
per ray is the exact sum of its ``spp`` radiances, rounded once and divided by ``spp``: three linear float64 values, NaN when a sample
was NaN, infinite or >= 2^31.  All compute happens in librtw_hip.so; there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _capi
from .rays import pack_rays
from .render import _record_stats
from .structs import flatten_scene


def make_trace_params(*, spp, max_depth=16, seed=1, first_stream=0, first_sample=0, flags=0, device=-1, max_workgroups=0, numerics=None):
    """``rtw_trace_params``.  ``numerics`` as in ``_capi.make_params``: a mode's name, or None = the module default; ``flags`` may name the
    mode instead (naming a DIFFERENT mode both ways is a ValueError)."""
    flags = int(flags)
    named = flags & (_capi.FLAG_NUMERICS_CONTRACT | _capi.FLAG_NUMERICS_REFERENCE_FMA2)
    if not named:
        flags |= _capi.numerics_flags(numerics)
    elif numerics is not None and _capi.numerics_flags(numerics) != named:
        raise ValueError(f"numerics={numerics!r} conflicts with the NUMERICS bit already in flags (0x{named:x})")
    return _capi.TraceParams(flags, int(device), int(max_workgroups), int(spp), int(max_depth), 0, int(seed), int(first_stream), int(first_sample))


def trace_rays(scene, rays, *, spp, max_depth=16, seed=1, first_stream=0, first_sample=0, T=np.float32, flags=0, max_workgroups=0,
               device=-1, numerics=None):
    """The radiance along every ray of ``rays`` (``rays.pack_rays``) in ``scene`` (a HittableList or the flat dict of ``flatten_scene``)
    through the host-buffer call (rtw_trace_rays_*): -> ``[n, 3]`` float64, linear.  ``flags``: RTW_FLAG_SCAN_VALU runs the scan on the
    vector ALUs, RTW_FLAG_GROUP_CULL is accepted and changes nothing.  ``max_workgroups``: a cap on the launch grid (scheduling only).
    A list traced in two calls, the second with ``first_stream`` advanced by the first call's length, gives the words of one call."""
    T = np.dtype(T).type
    if np.dtype(T) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("T must be float32 or float64")
    L = _capi.lib()
    packed = pack_rays(rays, T)
    n = packed.shape[0]
    flat = scene if isinstance(scene, dict) else flatten_scene(scene, T)
    S, keep = _capi.make_scene(flat, T)
    P = make_trace_params(spp=spp, max_depth=max_depth, seed=seed, first_stream=first_stream, first_sample=first_sample, flags=flags,
                          device=device, max_workgroups=max_workgroups, numerics=numerics)
    out = np.empty((n, 3), dtype=np.float64)
    fn = getattr(L, "rtw_trace_rays_" + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(C.byref(S), packed.ctypes.data_as(C.c_void_p), n, C.byref(P), out.ctypes.data_as(C.c_void_p)))
    del keep
    if n:
        _record_stats(L)
    return out


def trace_rays_into(scene_handle, d_rays_ptr, n, d_out_ptr, *, spp, max_depth=16, seed=1, first_stream=0, first_sample=0, T=np.float32,
                    flags=0, stream=0, max_workgroups=0, numerics=None):
    """The device-resident form (rtw_trace_rays_device_*; ``DeviceRenderer.trace_rays_into``): enqueue ONE launch over the ``n`` rays at
    ``d_rays_ptr`` (n * 8 elements of ``T``, 16-byte aligned) of the uploaded scene ``scene_handle`` on ``stream``; the results go to
    ``d_out_ptr`` (n * 3 float64, 8-byte aligned)."""
    L = _capi.lib()
    P = make_trace_params(spp=spp, max_depth=max_depth, seed=seed, first_stream=first_stream, first_sample=first_sample, flags=flags,
                          device=-1, max_workgroups=max_workgroups, numerics=numerics)
    fn = getattr(L, "rtw_trace_rays_device_" + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(scene_handle, C.c_void_p(int(d_rays_ptr)), int(n), C.byref(P), C.c_void_p(int(d_out_ptr)), C.c_void_p(int(stream))))
