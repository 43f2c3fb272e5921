"""Wide apertures (include/rtw_hip.h ``rtw_wide_aperture_*``): depth of field with circles of confusion up to 32 px.  The defocus stage
(``defocus.py``) clamps every circle at 8 px; at 1920 x 1080 the headline camera's far field is 15 px wide.  This stage runs that stage
as it is for what is nearly sharp, gathers a copy of the frame reduced by 2 (``max_radius`` 9..16) or 4 (17..32) with the same gather for
what is wide, and blends the two by the radius (from 4 px, the narrow result alone, to 8 px, the wide one alone).  With ``max_radius <= 8``
it IS the defocus stage, on the bits.  The definition is in the header; tests/wide_aperture_ref.py restates it on the CPU, twice, and the
device agrees on the bits.  All compute happens in librtw_hip.so; there is no CPU fallback.

Batches (``rtw_lens_batch_*``): ``wide_aperture_batch`` runs N views, ``focus_bracket`` ONE frame under N lenses, in the same six
launches; ``render_wide_aperture_batch`` is the one-call form for N cameras.  View ``v`` is the single call on the bits.

Defaults: ``max_radius=32, focus_dist=0`` (the camera's own focus plane), ``gamma=True``; what they buy on the CPU witness: DESIGN.md section 7.27.
"""
import ctypes as C

import numpy as np

from . import _capi
from .defocus import _entry, _host_arrays, _lens_arrays, _render_lens, _stage_host, _stage_into
from .render import _batch_cameras


def make_wide_aperture(lens_radius, focus_dist=0.0, max_radius=32, gamma=True, device=-1):
    """-> the ``rtw_wide_aperture_t`` of these keywords: those of ``make_defocus`` with ``max_radius`` in 1..32"""
    return _capi.WideAperture(int(max_radius), 0, 1 if gamma else 0, int(device), (C.c_int32 * 2)(0, 0), float(lens_radius), float(focus_dist))


def wide_aperture_work_bytes(image_width, image_height, elem_type=np.float32, max_radius=32):
    """bytes of the caller-owned workspace (the header lists its regions); for ``max_radius <= 8`` what ``defocus_work_bytes`` reports"""
    n = _capi.lib().rtw_wide_aperture_work_bytes(int(image_width), int(image_height), np.dtype(elem_type).itemsize, int(max_radius))
    if n < 0:
        _capi.check(int(n))
    return int(n)


def wide_aperture(image, features, cam, **params):
    """The stage on host arrays (rtw_wide_aperture_*): ``image`` [H, W, 3] (linear, rendered through the pinhole) and ``features`` [H, W, 8]
    -- or the dict ``render_features`` returns -- of the frame seen through ``cam``, whose own ``lens_radius`` is not read: the aperture is
    the keyword.  -> the image [H, W, 3]; a pixel that is not valid is NaN.  Keywords: ``make_wide_aperture``.  Blocking."""
    return _stage_host("rtw_wide_aperture_", make_wide_aperture, image, features, cam, params)


def wide_aperture_into(d_out_ptr, d_work_ptr, d_image_ptr, d_features_ptr, cam, image_width, image_height, *, elem_type=np.float32, stream=0, **params):
    """The device-resident stage (rtw_wide_aperture_device_*): six launches on ``stream`` (two when ``max_radius <= 8``).  DEVICE pointers in
    the library's layout (pixel (i, j) at slot ``j*H + i``): the linear image and the features; ``d_work_ptr``: ``wide_aperture_work_bytes``
    bytes for the same ``max_radius``, 16-byte aligned, which afterwards hold the regions the header lists; ``d_out_ptr`` aliases nothing.
    Keywords: ``make_wide_aperture``."""
    _stage_into("rtw_wide_aperture_device_", make_wide_aperture, d_out_ptr, d_work_ptr, d_image_ptr, d_features_ptr, cam, image_width, image_height, elem_type, stream, params)


def render_wide_aperture(scene, cam, image_width=400, n_samples=1, *, depth=16, seed=1, n_chunks=0, device=-1, gamma=True, denoise=None, wide_aperture=None):
    """Render through the pinhole and apply the lens afterwards, in one call on the device (rtw_render_wide_aperture_*): ``render_defocused``
    with this stage at the end of the chain.  ``wide_aperture``: None, or a dict of ``make_wide_aperture``'s keywords ``lens_radius``
    (default: the camera's own), ``focus_dist``, ``max_radius``.  Returns ``img[i, j, :]`` -- on the bits the chain of the single calls on the
    pinhole copy followed by ``wide_aperture``; ``last_stats()`` reports the render."""
    return _render_lens("rtw_render_wide_aperture_", make_wide_aperture, "wide_aperture", wide_aperture, scene, cam, image_width, n_samples, depth, seed, n_chunks, device, gamma, denoise)


# ---- batched views and brackets (include/rtw_hip.h rtw_lens_batch_*): N views, or one frame under N lenses, in each launch ----------

def lens_table(cams, image_width, image_height, *, lens_radii=None, focus_dists=None, **params):
    """The HOST table of a batch's lenses (rtw_lens_table_*): [N, 32] elements of the cameras' type, row ``v`` the constants of ``cams[v]`` with
    ``lens_radii[v]`` and ``focus_dists[v]`` (None: the keywords ``lens_radius`` / ``focus_dist`` for every view).  The caller uploads it for
    ``wide_aperture_batch_into``.  Keywords: ``make_wide_aperture``."""
    cams, T = _batch_cameras(cams)
    n = len(cams)
    lr, fd = _lens_arrays(lens_radii, focus_dists, n)
    params.setdefault("lens_radius", 0.0)
    table = np.zeros((n, 32), dtype=T)
    fn = _entry("rtw_lens_table_", T)
    _capi.check(fn(C.byref(make_wide_aperture(**params)), _capi.make_cameras(cams, T), n, int(image_width), int(image_height), lr, fd, table.ctypes.data_as(C.c_void_p)))
    return table


def wide_aperture_batch_work_bytes(image_width, image_height, n_views, elem_type=np.float32, max_radius=32):
    """bytes of the batch's workspace: ``n_views`` single-stage workspaces one behind the other, each with the single stage's layout"""
    n = _capi.lib().rtw_lens_batch_work_bytes(int(image_width), int(image_height), np.dtype(elem_type).itemsize, int(max_radius), int(n_views))
    if n < 0:
        _capi.check(int(n))
    return int(n)


def _batch_host(images, features, cams, n_frames, lens_radii, focus_dists, params):
    T, img, feat = _host_arrays(images, features, batch=True)
    cams, Tc = _batch_cameras(cams)
    if np.dtype(Tc) != T:
        raise TypeError(f"the cameras have element type {np.dtype(Tc).name}, the frames {T.name}")
    n = len(cams)
    if img.shape[0] != n_frames:
        raise ValueError(f"{img.shape[0]} frames where {n_frames} are expected for {n} views")
    W, H = img.shape[1:3]
    lr, fd = _lens_arrays(lens_radii, focus_dists, n)
    params.setdefault("lens_radius", 0.0)
    out = np.empty((n, W, H, 3), dtype=T)
    _capi.check(_entry("rtw_lens_batch_", T)(C.byref(make_wide_aperture(**params)), _capi.make_cameras(cams, T.type), n, n_frames, lr, fd, W, H,
                                             *(a.ctypes.data_as(C.c_void_p) for a in (img, feat, out))))
    return np.swapaxes(out, 1, 2)


def wide_aperture_batch(images, features, cams, *, lens_radii=None, focus_dists=None, **params):
    """``images`` [N, H, W, 3] and ``features`` [N, H, W, 8] -- or the dict ``render_features_batch`` returns -- of N views seen through
    ``cams`` -> the N images [N, H, W, 3] in six launches for all views, two when ``max_radius <= 8`` (rtw_lens_batch_*).
    ``lens_radii`` / ``focus_dists``: per-view sequences (None: the keywords ``lens_radius`` / ``focus_dist`` for every view).  View ``v`` is
    bit for bit ``wide_aperture(images[v], features[v], cams[v], lens_radius=lens_radii[v], focus_dist=focus_dists[v], ...)``.  Keywords:
    ``make_wide_aperture``.  Blocking; ``last_stats()`` is left as it was."""
    cams = list(cams)
    return _batch_host(images, features, cams, len(cams), lens_radii, focus_dists, params)


def focus_bracket(image, features, cam, *, focus_dists=None, lens_radii=None, **params):
    """ONE frame under N lenses in one call (rtw_lens_batch_* with ``n_frames == 1``): ``image`` [H, W, 3] and ``features``
    [H, W, 8] of the frame seen through ``cam``; ``focus_dists`` and/or ``lens_radii``: sequences of N values (one of them may be None: the
    keyword ``focus_dist`` / ``lens_radius`` for every lens) -> [N, H, W, 3].  Lens ``v`` is bit for bit ``wide_aperture(image, features, cam,
    lens_radius=lens_radii[v], focus_dist=focus_dists[v], ...)``.  Keywords: ``make_wide_aperture``.  Blocking."""
    if focus_dists is None and lens_radii is None:
        raise ValueError("a bracket needs focus_dists, lens_radii or both")
    n = len(list(focus_dists if focus_dists is not None else lens_radii))
    if n < 1:
        raise ValueError("a bracket needs at least one lens")
    if isinstance(features, dict):
        features = features["raw"]
    return _batch_host(np.asarray(image)[None], np.asarray(features)[None], [cam] * n, 1, lens_radii, focus_dists, params)


def wide_aperture_batch_into(d_out_ptr, d_work_ptr, d_images_ptr, d_features_ptr, d_table_ptr, image_width, image_height, n_views, *, n_frames=None, elem_type=np.float32,
                             stream=0, max_radius=32, gamma=True, device=-1):
    """The device-resident batched stage (rtw_lens_batch_device_*): six launches on ``stream`` (two when ``max_radius <= 8``) for
    ``n_views`` views.  DEVICE pointers: ``d_table_ptr`` the uploaded ``lens_table`` (16-byte aligned; the per-view lens lives there), the
    images and features of ``n_frames`` frames (``n_views``, the default, or 1: every view reads frame 0), ``d_work_ptr`` of
    ``wide_aperture_batch_work_bytes`` bytes and ``d_out_ptr`` of ``n_views`` frames, views one behind the other."""
    T = np.dtype(elem_type).type
    fn = _entry("rtw_lens_batch_device_", T)
    B = make_wide_aperture(0.0, 0.0, max_radius, gamma, device)
    _capi.check(fn(C.byref(B), int(n_views), int(n_views if n_frames is None else n_frames), C.c_void_p(int(d_table_ptr)), int(image_width), int(image_height),
                   *(C.c_void_p(int(q)) for q in (d_images_ptr, d_features_ptr, d_work_ptr, d_out_ptr)), C.c_void_p(int(stream))))


def render_wide_aperture_batch(scene, cams, image_width=400, n_samples=1, *, seeds=None, depth=16, seed=1, n_chunks=0, device=-1, gamma=True, denoise=None, wide_aperture=None,
                               lens_radii=None, focus_dists=None):
    """``render_wide_aperture`` for N cameras in one call (rtw_render_lens_batch_*): one batched render and one batched feature
    pass through the pinhole copies, with ``denoise`` one batched filter pass, then the batched lens stage; the result comes back once.
    Returns ``img[v, i, j, :]``; view ``v`` is bit for bit ``render_wide_aperture(scene, cams[v], ..., seed=seeds[v])`` with
    ``lens_radii[v]`` (default: the camera's own) and ``focus_dists[v]``.  ``last_stats()`` reports the render."""
    return _render_lens("rtw_render_lens_batch_", make_wide_aperture, "wide_aperture", wide_aperture, scene, cams, image_width, n_samples, depth, seed, n_chunks, device, gamma, denoise,
                        batch=(seeds, lens_radii, focus_dists))
