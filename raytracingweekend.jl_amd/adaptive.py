"""Adaptive sampling: a progressive render that stops each 8x8 tile at an exact noise estimate (include/rtw_hip.h
``rtw_render_adaptive_*``; the definition is in that header and in DESIGN.md).

Every tile ``t`` (column-major, ``t = tj * tiles_i + ti``) ends up holding a prefix ``[0, C_t)`` of the render's chunks, and its pixels
equal, bit for bit, those of ``render(...)`` with ``n_samples = min(S, C_t * chunk size), n_chunks = C_t``.  ``C_t`` is the first
checkpoint at which the tile's half-difference statistic passes the stopping rule.  All compute happens in librtw_hip.so; the only
arithmetic here is ``reference_decisions``, a plain restatement of the rule that the tests use as their witness.
"""
import ctypes as C

import numpy as np

from . import _capi
from .progressive import ProgressiveBatchRenderer, ProgressiveRenderer

#: Default ``dark_floor``: 1 % of a white pixel (R + G + B = 3 per sample).  A CHOICE, not a measurement: it says below which
#: brightness a tile's relative error stops mattering, and a caller who cares about deep shadows lowers it.
DEFAULT_DARK_FLOOR = 0.03


def default_check_chunks(n_chunks):
    """the library's default for ``min_chunks`` and ``check_chunks``: the smallest even number >= max(16, N / 8)"""
    m = max(16, (int(n_chunks) + 7) // 8)
    return m + (m & 1)


def checkpoints(n_chunks, min_chunks=0, check_chunks=0):
    """the chunk counts at which tiles are tested: ``min_chunks, min_chunks + check_chunks, ...`` below ``n_chunks``"""
    n = int(n_chunks)
    first = int(min_chunks) or default_check_chunks(n)
    step = int(check_chunks) or default_check_chunks(n)
    return list(range(first, n, step))


def _signed128(lo, hi):
    v = int(lo) | (int(hi) << 64)
    return v - (1 << 128) if v >> 127 else v


def _signed64(w):
    v = int(w)
    return v - (1 << 64) if v >> 63 else v


def noise_q(x):
    """The noise statistic of one channel value ``x`` (a binary64 radiance): ``min(fx >> 40, 2^30 - 1)`` with ``fx`` the value in
    64.64 fixed point, truncated towards zero, as the kernel adds it; 0 for a negative, non-finite or out-of-range value."""
    from fractions import Fraction
    x = float(x)
    if not (abs(x) < 2147483648.0) or x < 0:
        return 0
    return min(int(Fraction(x) * 2 ** 64) >> 40, 2 ** 30 - 1)


def reference_decisions(words, width, height, n, tol, floor, return_terms=False):
    """The stopping rule, evaluated from accumulator words in Python integers and binary64 floats exactly as it is written.

    ``words[i, j, :]`` (``H x W x 8`` uint64, what ``read_pixels`` returns) of an accumulator whose every pixel holds ``n`` samples.
    Returns a bool array over the tiles, ``converged[t]`` with ``t = tj * tiles_i + ti``; with ``return_terms`` also the lists
    ``D``, ``Y`` and ``M = max(Y, floor * n * npix)`` per tile."""
    H, W = int(height), int(width)
    words = np.asarray(words)
    assert words.shape == (H, W, 8)
    tiles_i, tiles_j = (H + 7) // 8, (W + 7) // 8
    tol, floor = float(tol), float(floor)
    conv, Ds, Ys, Ms = [], [], [], []
    for tj in range(tiles_j):
        for ti in range(tiles_i):
            D = Y = 0.0
            npix = 0
            for l in range(64):                                   # tile-local order (i & 7) + 8 * (j & 7)
                i, j = ti * 8 + (l & 7), tj * 8 + (l >> 3)
                if i >= H or j >= W:
                    continue
                npix += 1
                w = words[i, j]
                if int(w[6]) != 0:                                # poisoned: adds 0 to both sums
                    continue
                D = D + float(abs(_signed64(w[7]))) * 2.0 ** -24
                y = (_signed128(w[0], w[1]) / 2 ** 64 + _signed128(w[2], w[3]) / 2 ** 64) + _signed128(w[4], w[5]) / 2 ** 64
                Y = Y + max(y, 0.0)
            M = max(Y, (floor * float(n)) * float(npix))
            conv.append(D <= tol * M)
            Ds.append(D); Ys.append(Y); Ms.append(M)
    conv = np.array(conv, dtype=bool)
    return (conv, Ds, Ys, Ms) if return_terms else conv


class AdaptiveRenderer(ProgressiveRenderer):
    """One adaptive render of at most ``n_samples`` samples per pixel.  ``run(tolerance)`` renders until every tile is converged
    under ``tolerance`` or holds all chunks (blocking); calling it again with a smaller tolerance REFINES: the result is that of a
    fresh run at the new tolerance.  ``dark_floor``, ``min_chunks`` and ``check_chunks`` belong to the render and stay fixed;
    ``group_cull`` / ``scan_valu`` / ``job_pixels`` may differ from run to run (they do not change the image).

    The plain passes of the parent class (``add``, ``add_range``, ``merge``, ``save``) are refused by the library once the
    accumulator is adaptive (RtwError -2); ``reset()`` makes it a plain one again."""

    def __init__(self, scene, cam, image_width=400, n_samples=1, *, dark_floor=DEFAULT_DARK_FLOOR, min_chunks=0, check_chunks=0,
                 depth=16, seed=1, n_chunks=0, device=-1, numerics=None):
        super().__init__(scene, cam, image_width, n_samples, depth=depth, seed=seed, n_chunks=n_chunks, device=device, numerics=numerics)
        self.dark_floor, self.min_chunks, self.check_chunks = float(dark_floor), int(min_chunks), int(check_chunks)

    @property
    def tiles(self):
        """(tiles down a column, tiles along a row)"""
        return (self.height + 7) // 8, (self.width + 7) // 8

    def run(self, tolerance, *, group_cull=False, scan_valu=False, job_pixels=0, d_out=None, gamma=True, stream=0):
        """Render to ``tolerance`` (blocking).  ``d_out``: a device pointer that receives the final image.  Returns ``info()``."""
        flags = (_capi.FLAG_GROUP_CULL if group_cull else 0) | (_capi.FLAG_SCAN_VALU if scan_valu else 0)
        P = _capi.make_params(self.width, self.height, self.n_samples, self.depth, self.seed, self._n_chunks_arg, 0, 1, -1,
                              1 if gamma else 0, flags, job_pixels=job_pixels, numerics=self.numerics)
        A = _capi.Adaptive(float(tolerance), self.dark_floor, self.min_chunks, self.check_chunks)
        fn = self.L.rtw_render_adaptive_f64 if _capi.is_f64(self.T) else self.L.rtw_render_adaptive_f32
        _capi.check(fn(self.handle, C.byref(self.cam), C.byref(P), C.byref(A), self.accum,
                       C.c_void_p(int(d_out)) if d_out else None, C.c_void_p(int(stream))))
        return self.info()

    def tile_chunks(self):
        """``C_t`` as an int32 array of shape (tiles_i, tiles_j): ``[ti, tj]`` = the chunks tile ``tj * tiles_i + ti`` holds"""
        ti, tj = self.tiles
        buf = np.zeros(ti * tj, dtype=np.int32)
        n = C.c_int32(0)
        _capi.check(self.L.rtw_accum_tile_chunks(self.accum, buf.size, C.byref(n), buf.ctypes.data_as(C.POINTER(C.c_int32))))
        assert n.value == buf.size
        return buf.reshape(tj, ti).T

    def samples_per_pixel(self):
        """int32 ``H x W``: the samples each pixel holds, ``min(n_samples, C_t * chunk size)`` of its tile"""
        spp = np.minimum(self.n_samples, self.tile_chunks().astype(np.int64) * self.chunk_spp).astype(np.int32)
        return np.repeat(np.repeat(spp, 8, axis=0), 8, axis=1)[:self.height, :self.width]

    def noise_into(self, d_out_ptr, stream=0):
        """Enqueue the noise map (rtw_accum_noise_*) into device memory at ``d_out_ptr``: H*W elements, pixel (i, j) at ``j*H + i``."""
        fn = self.L.rtw_accum_noise_f64 if _capi.is_f64(self.T) else self.L.rtw_accum_noise_f32
        _capi.check(fn(self.accum, C.c_void_p(int(d_out_ptr)), C.c_void_p(int(stream))))

    def noise(self):
        """``H x W``: the per-pixel relative noise of the render so far -- the 3x3 binomial mean of ``|H_p| 2^-24 / max(y_p, dark_floor
        n)``, the stopping rule's own quantities for one pixel; NaN for a poisoned pixel (blocking)."""
        import torch
        buf = self._device_buffer(self.height * self.width)
        self.noise_into(buf.data_ptr(), stream=torch.cuda.current_stream(buf.device).cuda_stream)
        return buf.cpu().numpy().reshape(self.width, self.height).T

    def denoised(self, guided=True, gamma=True, **params):
        """The adaptive image filtered with the features of exactly the samples each tile holds (rtw_accum_filtered_*, blocking).
        ``guided`` (default): the colour weight of every pixel is scaled by its own noise estimate (``noise()``), so ``sigma_color``
        counts standard deviations (default ``GUIDED_SIGMA_COLOR``); ``guided=False``: the plain filter.  Keywords: ``make_denoise``."""
        if guided:
            from .denoise import GUIDED_SIGMA_COLOR
            params.setdefault("sigma_color", GUIDED_SIGMA_COLOR)
        return self._filtered(bool(guided), gamma, params)

    def info(self):
        """the accumulator's info (``samples_done`` / ``chunks_done``: the least sampled tile) and, once a run has finished, the
        fields of ``rtw_adaptive_info_t``"""
        out = super().info()
        st = _capi.AdaptiveInfo()
        if self.L.rtw_accum_adaptive_info(self.accum, C.byref(st)) == 0:
            out.update({k: getattr(st, k) for k, _ in st._fields_})
        return out


def render_adaptive_denoised(scene, cam, image_width=400, n_samples=1, *, tolerance, guided=True, dark_floor=DEFAULT_DARK_FLOOR, depth=16, seed=1,
                             n_chunks=0, min_chunks=0, check_chunks=0, group_cull=False, scan_valu=False, numerics=None, gamma=True, device=-1,
                             **denoise_params):
    """``render_adaptive`` followed by ``AdaptiveRenderer.denoised`` on the device: every tile is filtered with the features of the
    chunks it holds and, with ``guided`` (default), with a colour weight scaled by each pixel's own noise estimate.  ``denoise_params``:
    the keywords of ``make_denoise`` but ``gamma`` / ``device``.  Returns ``(image, samples_per_pixel, info)`` like ``render_adaptive``."""
    with AdaptiveRenderer(scene, cam, image_width, n_samples, dark_floor=dark_floor, min_chunks=min_chunks, check_chunks=check_chunks,
                          depth=depth, seed=seed, n_chunks=n_chunks, device=device, numerics=numerics) as ar:
        info = ar.run(tolerance, group_cull=group_cull, scan_valu=scan_valu)
        return ar.denoised(guided=guided, gamma=gamma, **denoise_params), ar.samples_per_pixel(), info


def render_adaptive(scene, cam, image_width=400, n_samples=1, *, tolerance, dark_floor=DEFAULT_DARK_FLOOR, depth=16, seed=1, n_chunks=0,
                    min_chunks=0, check_chunks=0, group_cull=False, scan_valu=False, numerics=None, gamma=True, device=-1):
    """``render(...)`` with at most ``n_samples`` samples per pixel, each 8x8 tile stopping at the first checkpoint at which it is
    converged under ``tolerance`` (roughly 0.8 x the tile's relative standard error -- an approximation; the exact rule is in
    include/rtw_hip.h).  ``dark_floor`` (default 0.03 = 1 % of white, a choice and not a measurement) is the radiance per sample
    and pixel, summed over the channels, below which a tile is judged as if it were that bright.

    Returns ``(image, samples_per_pixel, info)``: the image like ``render``'s, an int32 ``H x W`` map of the samples each pixel
    holds, and the dict of ``AdaptiveRenderer.info()``."""
    with AdaptiveRenderer(scene, cam, image_width, n_samples, dark_floor=dark_floor, min_chunks=min_chunks, check_chunks=check_chunks,
                          depth=depth, seed=seed, n_chunks=n_chunks, device=device, numerics=numerics) as ar:
        info = ar.run(tolerance, group_cull=group_cull, scan_valu=scan_valu)
        return ar.image(gamma=gamma), ar.samples_per_pixel(), info


class AdaptiveBatchRenderer(ProgressiveBatchRenderer):
    """N adaptive renders of ONE scene (a camera and a seed per view) run as one loop (``rtw_render_adaptive_batch_*``): per checkpoint
    one check, one list of the active tiles of all views, one host wait and one pass -- ``rounds`` launches and waits instead of
    N x ``rounds``.  View ``v`` is, bit for bit, the ``AdaptiveRenderer`` of ``cams[v]`` and ``seeds[v]``.  ``run`` again with a smaller
    tolerance refines every view."""

    def __init__(self, scene, cams, image_width=400, n_samples=1, *, dark_floor=DEFAULT_DARK_FLOOR, min_chunks=0, check_chunks=0,
                 depth=16, seeds=1, n_chunks=0, device=-1, numerics=None):
        super().__init__(scene, cams, image_width, n_samples, depth=depth, seeds=seeds, n_chunks=n_chunks, device=device, numerics=numerics)
        self.dark_floor, self.min_chunks, self.check_chunks = float(dark_floor), int(min_chunks), int(check_chunks)

    @property
    def tiles(self):
        """(tiles down a column, tiles along a row) of one view"""
        return (self.height + 7) // 8, (self.width + 7) // 8

    def run(self, tolerance, *, group_cull=False, scan_valu=False, job_pixels=0, d_out=None, gamma=True, stream=0):
        """Render every view to ``tolerance`` (blocking).  ``d_out``: a device pointer that receives the N final images.  Returns the
        list of ``info(v)``."""
        P = self._params(group_cull, scan_valu, job_pixels, gamma)
        A = _capi.Adaptive(float(tolerance), self.dark_floor, self.min_chunks, self.check_chunks)
        fn = self.L.rtw_render_adaptive_batch_f64 if _capi.is_f64(self.T) else self.L.rtw_render_adaptive_batch_f32
        _capi.check(fn(self.handle, self.cams, self.n_views, self.seeds, C.byref(P), C.byref(A), self._handles,
                       C.c_void_p(int(d_out)) if d_out else None, C.c_void_p(int(stream))))
        return [self.info(v) for v in range(self.n_views)]

    def tile_chunks(self):
        """``C_t`` as an int32 array of shape (N, tiles_i, tiles_j): ``[v, ti, tj]`` = the chunks tile ``tj * tiles_i + ti`` of view
        ``v`` holds"""
        ti, tj = self.tiles
        out = np.zeros((self.n_views, ti, tj), dtype=np.int32)
        for v, acc in enumerate(self.accums):
            buf = np.zeros(ti * tj, dtype=np.int32)
            n = C.c_int32(0)
            _capi.check(self.L.rtw_accum_tile_chunks(acc, buf.size, C.byref(n), buf.ctypes.data_as(C.POINTER(C.c_int32))))
            assert n.value == buf.size
            out[v] = buf.reshape(tj, ti).T
        return out

    def samples_per_pixel(self):
        """int32 ``N x H x W``: the samples each pixel of each view holds"""
        spp = np.minimum(self.n_samples, self.tile_chunks().astype(np.int64) * self.chunk_spp).astype(np.int32)
        return np.repeat(np.repeat(spp, 8, axis=1), 8, axis=2)[:, :self.height, :self.width]

    def denoised(self, v, guided=True, gamma=True, **params):
        """View ``v``'s adaptive image, filtered like ``AdaptiveRenderer.denoised``"""
        if guided:
            from .denoise import GUIDED_SIGMA_COLOR
            params.setdefault("sigma_color", GUIDED_SIGMA_COLOR)
        return self._filtered(v, bool(guided), gamma, params)

    def noise_all_into(self, d_out_ptr, stream=0):
        """Enqueue ONE noise-map launch for all views (rtw_accum_noise_batch_*) into device memory at ``d_out_ptr``: N*H*W elements, view
        ``v``'s map at ``v*H*W``, pixel (i, j) at ``j*H + i``."""
        fn = getattr(self.L, "rtw_accum_noise_batch_" + self._sfx())
        _capi.check(fn(self._handles, self.n_views, C.c_void_p(int(d_out_ptr)), C.c_void_p(int(stream))))

    def noise_all(self):
        """``N x H x W``: ``AdaptiveRenderer.noise()`` of every view (blocking)"""
        import torch
        buf = self._device_buffer(self.n_views * self.height * self.width)
        self.noise_all_into(buf.data_ptr(), stream=torch.cuda.current_stream(buf.device).cuda_stream)
        return buf.cpu().numpy().reshape(self.n_views, self.width, self.height).transpose(0, 2, 1)

    def denoised_all(self, guided=True, gamma=True, **params):
        """``denoised(v)`` of every view, ``[N, H, W, 3]``, in 4 + ``levels`` launches and one copy for any N (rtw_accum_filtered_batch_*, blocking)."""
        if guided:
            from .denoise import GUIDED_SIGMA_COLOR
            params.setdefault("sigma_color", GUIDED_SIGMA_COLOR)
        return self._filtered_all(bool(guided), gamma, params)

    def info(self, v):
        """view ``v``'s accumulator info and, once a run has finished, the fields of ``rtw_adaptive_info_t``"""
        out = super().info(v)
        st = _capi.AdaptiveInfo()
        if self.L.rtw_accum_adaptive_info(self.accums[v], C.byref(st)) == 0:
            out.update({k: getattr(st, k) for k, _ in st._fields_})
        return out


def render_adaptive_batch(scene, cams, image_width=400, n_samples=1, *, tolerance, seeds=None, dark_floor=DEFAULT_DARK_FLOOR, depth=16,
                          n_chunks=0, min_chunks=0, check_chunks=0, group_cull=False, scan_valu=False, numerics=None, gamma=True, device=-1):
    """``render_adaptive`` for N cameras of one scene in one loop of batched passes; view ``v`` equals ``render_adaptive(scene, cams[v],
    ..., seed=seeds[v])`` bit for bit.  ``seeds``: None (seed 1 for every view, ``render_adaptive``'s default), one int, or N ints.

    Returns ``(images, samples_per_pixel, infos)``: ``N x H x W x 3``, int32 ``N x H x W``, and the list of the views' info dicts."""
    with AdaptiveBatchRenderer(scene, cams, image_width, n_samples, dark_floor=dark_floor, min_chunks=min_chunks, check_chunks=check_chunks,
                               depth=depth, seeds=1 if seeds is None else seeds, n_chunks=n_chunks, device=device, numerics=numerics) as ar:
        infos = ar.run(tolerance, group_cull=group_cull, scan_valu=scan_valu)
        return ar.images(gamma=gamma), ar.samples_per_pixel(), infos


def render_adaptive_denoised_batch(scene, cams, image_width=400, n_samples=1, *, tolerance, guided=True, seeds=None, dark_floor=DEFAULT_DARK_FLOOR,
                                   depth=16, n_chunks=0, min_chunks=0, check_chunks=0, group_cull=False, scan_valu=False, numerics=None, gamma=True,
                                   device=-1, **denoise_params):
    """``render_adaptive_batch`` followed by ``AdaptiveBatchRenderer.denoised_all`` on the device; view ``v`` equals
    ``render_adaptive_denoised(scene, cams[v], ..., seed=seeds[v])`` bit for bit.  Returns ``(images, samples_per_pixel, infos)`` like
    ``render_adaptive_batch``."""
    with AdaptiveBatchRenderer(scene, cams, image_width, n_samples, dark_floor=dark_floor, min_chunks=min_chunks, check_chunks=check_chunks,
                               depth=depth, seeds=1 if seeds is None else seeds, n_chunks=n_chunks, device=device, numerics=numerics) as ar:
        infos = ar.run(tolerance, group_cull=group_cull, scan_valu=scan_valu)
        return ar.denoised_all(guided=guided, gamma=gamma, **denoise_params), ar.samples_per_pixel(), infos
