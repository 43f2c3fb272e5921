"""Ray queries (include/rtw_hip.h ``rtw_cast_rays_*``): the closest hit of caller-supplied rays against the whole sphere list -- the
intersection routine itself, for picking under a position that is no pixel centre, visibility and shadow tests between points,
line-of-sight queries, light baking or an integrator of the caller's own.

A ray is 8 elements ``ox oy oz dx dy dz tmax tag`` (``tag`` is the caller's and never read); the result per ray is the sphere's index in
the caller's list (-1: a miss) and, where asked for, the record ``t px py pz nx ny nz front`` of the reference's HitRecord, all +0 on a
miss.  The values are the reference's ``hit(::HittableList)`` with ``(tmin, tmax_i)`` on the bits: the later of two spheres with the same
root wins.  All compute happens in librtw_hip.so; there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _capi
from .render import _record_stats
from .structs import flatten_scene

RAY_ELEMS = 8     # elements of a ray and of a record


def make_rays_params(*, tmin=1e-4, flags=0, device=-1, max_workgroups=0, numerics=None):
    """``rtw_rays_params``.  ``numerics`` as in ``_capi.make_params``: a mode's name, or None = the module default; ``flags`` may name the
    mode instead (naming a DIFFERENT mode both ways is a ValueError)."""
    flags = int(flags)
    named = flags & (_capi.FLAG_NUMERICS_CONTRACT | _capi.FLAG_NUMERICS_REFERENCE_FMA2)
    if not named:
        flags |= _capi.numerics_flags(numerics)
    elif numerics is not None and _capi.numerics_flags(numerics) != named:
        raise ValueError(f"numerics={numerics!r} conflicts with the NUMERICS bit already in flags (0x{named:x})")
    return _capi.RaysParams(flags, int(device), int(max_workgroups), 0, float(tmin))


def pack_rays(rays, T=np.float32):
    """``rays`` [n, 8], or [n, 6] / [n, 7] padded with ``tmax = inf`` and ``tag = 0`` -> a C-contiguous [n, 8] array of ``T``"""
    a = np.asarray(rays)
    if a.ndim != 2 or a.shape[1] not in (6, 7, RAY_ELEMS):
        raise ValueError(f"rays must be [n, 6], [n, 7] or [n, 8], got {a.shape}")
    if a.shape[1] == RAY_ELEMS:
        return np.ascontiguousarray(a, dtype=T)
    out = np.zeros((a.shape[0], RAY_ELEMS), dtype=T)
    out[:, :a.shape[1]] = a
    if a.shape[1] == 6:
        out[:, 6] = np.inf
    return out


def cast_rays(scene, rays, *, tmin=1e-4, T=np.float32, flags=0, records=True, max_workgroups=0, device=-1, numerics=None):
    """The closest hit of every ray of ``rays`` (``pack_rays``) in ``scene`` (a HittableList or the flat dict of ``flatten_scene``) through
    the host-buffer call (rtw_cast_rays_*): -> ``(idx [n] int32, rec [n, 8] of T)``, ``rec`` None with ``records=False`` (the occlusion
    query: it pays the full scan).  ``flags``: RTW_FLAG_SCAN_VALU runs the scan on the vector ALUs, RTW_FLAG_GROUP_CULL is accepted and
    changes nothing.  ``max_workgroups``: a cap on the launch grid (scheduling only)."""
    T = np.dtype(T).type
    if np.dtype(T) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("T must be float32 or float64")
    L = _capi.lib()
    packed = pack_rays(rays, T)
    n = packed.shape[0]
    flat = scene if isinstance(scene, dict) else flatten_scene(scene, T)
    S, keep = _capi.make_scene(flat, T)
    P = make_rays_params(tmin=tmin, flags=flags, device=device, max_workgroups=max_workgroups, numerics=numerics)
    idx = np.empty(n, dtype=np.int32)
    rec = np.empty((n, RAY_ELEMS), dtype=T) if records else None
    fn = getattr(L, "rtw_cast_rays_" + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(C.byref(S), packed.ctypes.data_as(C.c_void_p), n, C.byref(P), idx.ctypes.data_as(C.c_void_p),
                   rec.ctypes.data_as(C.c_void_p) if records else None))
    del keep
    if n:
        _record_stats(L)
    return idx, rec


def cast_rays_into(scene_handle, d_rays_ptr, n, d_idx_ptr, d_rec_ptr, *, tmin=1e-4, T=np.float32, flags=0, stream=0, max_workgroups=0, numerics=None):
    """The device-resident form (rtw_cast_rays_device_*; ``DeviceRenderer.cast_rays_into``): enqueue ONE launch over the ``n`` rays at
    ``d_rays_ptr`` (n * 8 elements of ``T``, 16-byte aligned) of the uploaded scene ``scene_handle`` on ``stream``; the indices go to
    ``d_idx_ptr`` (n int32), the records to ``d_rec_ptr`` (n * 8 elements, 16-byte aligned; 0 / None: none)."""
    L = _capi.lib()
    P = make_rays_params(tmin=tmin, flags=flags, device=-1, max_workgroups=max_workgroups, numerics=numerics)
    fn = getattr(L, "rtw_cast_rays_device_" + ("f64" if _capi.is_f64(T) else "f32"))
    _capi.check(fn(scene_handle, C.c_void_p(int(d_rays_ptr)), int(n), C.byref(P), C.c_void_p(int(d_idx_ptr)),
                   C.c_void_p(int(d_rec_ptr)) if d_rec_ptr else None, C.c_void_p(int(stream))))
