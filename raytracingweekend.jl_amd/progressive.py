"""Progressive render: a render added up pass by pass in an exact accumulator (include/rtw_hip.h ``rtw_accum_*``).

Any partition of a render's chunks into passes -- in any order, scan mode or job size, on one accumulator or merged from several --
resolves to the image of the single ``render(...)`` call, bit for bit; every prefix ``[0, C)`` is itself the render with
``n_samples = min(S, C * chunk size), n_chunks = C``.  All compute happens in librtw_hip.so; there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _capi
from .render import _as_image
from .structs import Camera, flatten_scene, image_height


def effective_chunks(spp, n_chunks=0):
    """``(effective n_chunks, samples per chunk)`` of a render: the library's rule (``rtw_params.n_chunks``; 0 = ``min(spp, 256)``)."""
    spp, n_chunks = int(spp), int(n_chunks)
    if spp <= 0 or n_chunks < 0:
        raise ValueError("spp must be >= 1 and n_chunks >= 0")
    nch = min(n_chunks if n_chunks > 0 else min(spp, 256), spp)
    cs = (spp + nch - 1) // nch
    return (spp + cs - 1) // cs, cs


def samples_in_chunks(spp, n_chunks, begin, count):
    """Samples per pixel in the chunks ``[begin, begin + count)`` of a render of ``spp`` samples in ``n_chunks`` chunks (the last chunk
    may be short).  Raises ValueError for a range outside the render's effective chunks."""
    nch, cs = effective_chunks(spp, n_chunks)
    begin, count = int(begin), int(count)
    if begin < 0 or count < 1 or begin + count > nch:
        raise ValueError(f"chunk range [{begin}, {begin + count}) is not inside the render's {nch} chunks")
    return min(int(spp), (begin + count) * cs) - min(int(spp), begin * cs)


_NUMERICS_OF_FLAGS = {flags: name for name, (flags, _) in _capi.NUMERICS.items()}


class ProgressiveRenderer:
    """One render of ``n_samples`` samples per pixel, rendered a chunk range at a time into an exact accumulator on the device.

    ``n_chunks`` keeps ``render``'s default (``min(n_samples, 256)``), so the finished image equals ``render(...)`` with the same
    arguments.  Open-ended refinement in 1-sample steps beyond 256 samples: pass ``n_chunks=n_samples`` (a large ``n_samples`` costs
    nothing until its chunks are rendered).

    ``add`` / ``add_range`` enqueue passes (asynchronous on ``stream``; operations on one renderer are ordered by the library);
    ``image`` resolves what has been added so far.  ``group_cull``, ``scan_valu`` and ``job_pixels`` may differ from pass to pass: they
    do not change the image."""

    def __init__(self, scene, cam, image_width=400, n_samples=1, *, depth=16, seed=1, n_chunks=0, device=-1, numerics=None):
        if not isinstance(cam, Camera):
            raise TypeError("cam must be a Camera")
        self.T = cam.elem_type
        self.width, self.height = int(image_width), image_height(image_width)
        if self.width <= 0 or self.height <= 0:
            raise ValueError(f"image_width={image_width} gives an empty {self.height} x {image_width} image")
        self.n_samples, self.depth, self.seed = int(n_samples), int(depth), int(seed)
        self.n_chunks, self.chunk_spp = effective_chunks(n_samples, n_chunks)          # (ValueError for n_samples < 1)
        self._n_chunks_arg = int(n_chunks)
        self.numerics = _capi.numerics_name(numerics)
        self.L = _capi.lib()
        self.handle, self.accum = C.c_void_p(), C.c_void_p()
        flat = flatten_scene(scene, self.T)
        S, keep = _capi.make_scene(flat, self.T)
        self.cam = _capi.make_camera(cam, self.T)
        up = self.L.rtw_scene_upload_f64 if _capi.is_f64(self.T) else self.L.rtw_scene_upload_f32
        _capi.check(up(C.byref(S), int(device), C.byref(self.handle)))
        del keep
        self._create_accum(device)

    def _create_accum(self, device):
        try:
            _capi.check(self.L.rtw_accum_create(int(device), self.width, self.height, C.byref(self.accum)))
        except Exception:
            self.close()
            raise

    # ---- passes ----
    def add_range(self, begin, count, *, group_cull=False, scan_valu=False, job_pixels=0, d_out=None, gamma=True, stream=0):
        """Enqueue the chunks ``[begin, begin + count)``; ``d_out``: a device pointer that receives the running image (H*W*3 elements).
        Returns ``samples_done``."""
        flags = (_capi.FLAG_GROUP_CULL if group_cull else 0) | (_capi.FLAG_SCAN_VALU if scan_valu else 0)
        P = _capi.make_params(self.width, self.height, self.n_samples, self.depth, self.seed, self._n_chunks_arg, 0, 1, -1,
                              1 if gamma else 0, flags, job_pixels=job_pixels, numerics=self.numerics)
        fn = self.L.rtw_render_accum_f64 if _capi.is_f64(self.T) else self.L.rtw_render_accum_f32
        _capi.check(fn(self.handle, C.byref(self.cam), C.byref(P), int(begin), int(count), self.accum,
                       C.c_void_p(int(d_out)) if d_out else None, C.c_void_p(int(stream))))
        return self.samples_done

    def add(self, n_chunks=1, **kw):
        """Enqueue the next ``n_chunks`` chunks not yet added (fewer at the end of the render or before chunks already there).
        Returns ``samples_done``; raises ValueError when the render is complete."""
        if int(n_chunks) < 1:
            raise ValueError("n_chunks must be >= 1")
        begin, room = self._first_gap()
        if room < 1:
            raise ValueError("the render is complete: every chunk has been added")
        return self.add_range(begin, min(int(n_chunks), room), **kw)

    def _first_gap(self):
        """(first chunk not yet added, how many chunks are free from there)"""
        rs = self.ranges()
        if not rs or rs[0][0] > 0:
            return 0, (rs[0][0] if rs else self.n_chunks)
        end = rs[0][1]
        return end, (rs[1][0] if len(rs) > 1 else self.n_chunks) - end

    def ranges(self):
        """the chunk ranges added so far: sorted list of ``(begin, end)``, end exclusive"""
        n = C.c_int32(0)
        _capi.check(self.L.rtw_accum_ranges(self.accum, 0, C.byref(n), None))
        buf = (C.c_int32 * (2 * max(n.value, 1)))()
        _capi.check(self.L.rtw_accum_ranges(self.accum, n.value, C.byref(n), buf))
        return [(int(buf[2 * k]), int(buf[2 * k + 1])) for k in range(n.value)]

    # ---- results ----
    def image(self, gamma=True):
        """The image of the samples added so far (blocking): ``img[i, j, :]`` like ``render``."""
        out = np.empty(self.height * self.width * 3, dtype=self.T)
        fn = self.L.rtw_accum_resolve_host_f64 if _capi.is_f64(self.T) else self.L.rtw_accum_resolve_host_f32
        _capi.check(fn(self.accum, 1 if gamma else 0, out.ctypes.data_as(C.c_void_p)))
        return _as_image(out, self.height, self.width)

    def resolve_into(self, d_ptr, gamma=True, stream=0):
        """Enqueue the resolve into device memory at ``d_ptr`` (H*W*3 elements of the camera's element type)."""
        fn = self.L.rtw_accum_resolve_f64 if _capi.is_f64(self.T) else self.L.rtw_accum_resolve_f32
        _capi.check(fn(self.accum, 1 if gamma else 0, C.c_void_p(int(d_ptr)), C.c_void_p(int(stream))))

    def read_pixels(self):
        """The accumulator itself (blocking): ``words[i, j, :]`` = r_lo, r_hi, g_lo, g_hi, b_lo, b_hi, poison, 0 as uint64."""
        out = np.empty(self.height * self.width * 8, dtype=np.uint64)
        _capi.check(self.L.rtw_accum_read_pixels(self.accum, out.ctypes.data_as(C.c_void_p)))
        return out.reshape(self.width, self.height, 8).transpose(1, 0, 2)

    # ---- the accumulator as the denoiser's input (include/rtw_hip.h rtw_accum_features_*, rtw_accum_filtered_*) ----
    def _render_params(self, gamma=True, group_cull=False, scan_valu=False, job_pixels=0):
        flags = (_capi.FLAG_GROUP_CULL if group_cull else 0) | (_capi.FLAG_SCAN_VALU if scan_valu else 0)
        return _capi.make_params(self.width, self.height, self.n_samples, self.depth, self.seed, self._n_chunks_arg, 0, 1, -1,
                                 1 if gamma else 0, flags, job_pixels=job_pixels, numerics=self.numerics)

    def _device_buffer(self, n_elems):
        """a torch tensor on the accumulator's device (torch is the package's plumbing for device memory; it must have initialised
        the GPU before the library did)"""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("torch sees no GPU: a host copy of a device-resident result needs torch for its device buffer")
        dev = self.info()["device"]
        return torch.empty(int(n_elems), dtype=torch.float64 if _capi.is_f64(self.T) else torch.float32, device=f"cuda:{dev}")

    def features_into(self, d_out_ptr, *, scan_valu=False, group_cull=False, job_pixels=0, stream=0):
        """Enqueue the feature pass over exactly the samples the accumulator holds (rtw_accum_features_*) into device memory at
        ``d_out_ptr``: H*W*8 elements, 16-byte aligned, the layout of ``features_into``.  A uniform accumulator must hold ONE chunk
        interval; an adaptive one gets, per tile, the features of the chunks ``[0, C_t)``."""
        P = self._render_params(True, group_cull, scan_valu, job_pixels)
        fn = self.L.rtw_accum_features_f64 if _capi.is_f64(self.T) else self.L.rtw_accum_features_f32
        _capi.check(fn(self.handle, C.byref(self.cam), C.byref(P), self.accum, C.c_void_p(int(d_out_ptr)), C.c_void_p(int(stream))))

    def features(self, **kw):
        """The first-hit features of the samples added so far (blocking): the dict of ``render_features``."""
        import torch
        from .features import FEATURE_CHANNELS, split
        buf = self._device_buffer(self.height * self.width * FEATURE_CHANNELS)
        self.features_into(buf.data_ptr(), stream=torch.cuda.current_stream(buf.device).cuda_stream, **kw)
        raw = buf.cpu().numpy()
        return split(raw.reshape(self.width, self.height, FEATURE_CHANNELS).transpose(1, 0, 2))

    def _filtered(self, guided, gamma, kw):
        from .denoise import make_denoise
        D = make_denoise(gamma=gamma, **kw)
        P = self._render_params(gamma)
        out = np.empty(self.height * self.width * 3, dtype=self.T)
        fn = self.L.rtw_accum_filtered_f64 if _capi.is_f64(self.T) else self.L.rtw_accum_filtered_f32
        _capi.check(fn(self.handle, C.byref(self.cam), C.byref(P), C.byref(D), self.accum, 1 if guided else 0, out.ctypes.data_as(C.c_void_p)))
        return _as_image(out, self.height, self.width)

    def denoised(self, gamma=True, **params):
        """The image of the samples added so far, filtered with the features of exactly those samples (rtw_accum_filtered_*, blocking):
        resolve, feature pass and filter stay on the device, the result comes back once.  Keywords: ``make_denoise``."""
        return self._filtered(False, gamma, params)

    def info(self):
        st = _capi.AccumInfo()
        _capi.check(self.L.rtw_accum_info(self.accum, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    @property
    def samples_done(self):
        return self.info()["samples_done"]

    @property
    def done(self):
        return bool(self.info()["complete"])

    def stats(self):
        """Counters / kernel time of the calling thread's last pass (waits for it)."""
        st = _capi.Stats()
        _capi.check(self.L.rtw_stats(C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    # ---- combining, checkpoints ----
    def merge(self, other, stream=0):
        """Add ``other``'s chunks to this renderer's (same render, disjoint chunks, same device); ``other`` is left as it is."""
        if not isinstance(other, ProgressiveRenderer):
            raise TypeError("other must be a ProgressiveRenderer")
        _capi.check(self.L.rtw_accum_merge(self.accum, other.accum, C.c_void_p(int(stream))))

    def save(self, path):
        """Write the accumulator and the render it belongs to (``rtw_accum_export``'s blob) to ``path`` (blocking)."""
        size = C.c_uint64(0)
        _capi.check(self.L.rtw_accum_export(self.accum, None, 0, C.byref(size)))
        buf = np.empty(size.value, dtype=np.uint8)
        _capi.check(self.L.rtw_accum_export(self.accum, buf.ctypes.data_as(C.c_void_p), size.value, C.byref(size)))
        with open(path, "wb") as f:
            f.write(buf.tobytes())

    @classmethod
    def load(cls, path, scene, cam, *, device=-1):
        """Continue a saved render: ``scene`` and ``cam`` must be the ones it was made with (the first pass after loading is refused
        otherwise, RtwError -4).  A truncated file or one of another version raises RtwError -2."""
        with open(path, "rb") as f:
            blob = np.frombuffer(f.read(), dtype=np.uint8)
        L = _capi.lib()
        acc = C.c_void_p()
        _capi.check(L.rtw_accum_import(int(device), blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(acc)))
        st = _capi.AccumInfo()
        _capi.check(L.rtw_accum_info(acc, C.byref(st)))
        try:
            if not st.bound:
                raise ValueError(f"{path} holds an accumulator without a render")
            if (st.precision == 64) != _capi.is_f64(cam.elem_type):
                raise TypeError(f"{path} is a Float{st.precision} render, the camera is not")
            if image_height(st.width) != st.height:
                raise ValueError(f"{path}: {st.height} x {st.width} is not a frame of this package's aspect ratio")
            # (n_chunks = the effective count reproduces the saved chunk size: effective_chunks is idempotent)
            self = cls(scene, cam, st.width, st.spp, depth=st.max_depth, seed=st.seed, n_chunks=st.n_chunks, device=st.device,
                       numerics=_NUMERICS_OF_FLAGS[st.numerics_flags])
        except Exception:
            L.rtw_accum_free(acc)
            raise
        L.rtw_accum_free(self.accum)
        self.accum = acc
        return self

    def reset(self, cam=None):
        """Zero the accumulator and forget what was added; ``cam``: continue with another camera (of the same element type)."""
        if cam is not None:
            if not isinstance(cam, Camera) or np.dtype(cam.elem_type) != np.dtype(self.T):
                raise TypeError("cam must be a Camera of the renderer's element type")
            self.cam = _capi.make_camera(cam, self.T)
        _capi.check(self.L.rtw_accum_reset(self.accum, None))

    def close(self):
        if getattr(self, "accum", None):
            self.L.rtw_accum_free(self.accum)
            self.accum = C.c_void_p()
        if getattr(self, "handle", None):
            self.L.rtw_scene_free(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ProgressiveBatchRenderer:
    """N views of ONE scene -- same size, samples, chunks and depth; a camera and a seed per view -- each with its own exact accumulator,
    every pass ONE kernel launch for all of them (``rtw_render_accum_batch_*``).  View ``v`` is, bit for bit, the
    ``ProgressiveRenderer`` of ``cams[v]`` and ``seeds[v]``: the same words, ranges and image after the same chunks.

    ``seeds``: one int for every view, or a sequence of N.  ``add_range`` enqueues the chunks ``[begin, begin + count)`` of every view
    (asynchronous on ``stream``); ``images()`` resolves what has been added so far; ``read_pixels(v)`` / ``info(v)`` / ``ranges(v)``
    look at one view."""

    def __init__(self, scene, cams, image_width=400, n_samples=1, *, depth=16, seeds=1, n_chunks=0, device=-1, numerics=None):
        cams = list(cams)
        if not cams or not all(isinstance(c, Camera) for c in cams):
            raise TypeError("cams must be a non-empty sequence of Camera")
        self.T = cams[0].elem_type
        if any(np.dtype(c.elem_type) != np.dtype(self.T) for c in cams):
            raise TypeError("the cameras of a batch share one element type")
        self.n_views = len(cams)
        self.width, self.height = int(image_width), image_height(image_width)
        if self.width <= 0 or self.height <= 0:
            raise ValueError(f"image_width={image_width} gives an empty {self.height} x {image_width} image")
        self.n_samples, self.depth = int(n_samples), int(depth)
        self.n_chunks, self.chunk_spp = effective_chunks(n_samples, n_chunks)          # (ValueError for n_samples < 1)
        self._n_chunks_arg = int(n_chunks)
        self.numerics = _capi.numerics_name(numerics)
        self.seeds = _capi.make_seeds(seeds, self.n_views)                           # (ValueError for a wrong count)
        self.cams = _capi.make_cameras(cams, self.T)
        self.L = _capi.lib()
        self.handle, self.accums = C.c_void_p(), []
        flat = flatten_scene(scene, self.T)
        S, keep = _capi.make_scene(flat, self.T)
        up = self.L.rtw_scene_upload_f64 if _capi.is_f64(self.T) else self.L.rtw_scene_upload_f32
        _capi.check(up(C.byref(S), int(device), C.byref(self.handle)))
        del keep
        try:
            for _ in range(self.n_views):
                acc = C.c_void_p()
                _capi.check(self.L.rtw_accum_create(int(device), self.width, self.height, C.byref(acc)))
                self.accums.append(acc)
        except Exception:
            self.close()
            raise
        self._handles = _capi.make_handles(self.accums)

    def _params(self, group_cull, scan_valu, job_pixels, gamma):
        flags = (_capi.FLAG_GROUP_CULL if group_cull else 0) | (_capi.FLAG_SCAN_VALU if scan_valu else 0)
        return _capi.make_params(self.width, self.height, self.n_samples, self.depth, 0, self._n_chunks_arg, 0, 1, -1,
                                 1 if gamma else 0, flags, job_pixels=job_pixels, numerics=self.numerics)

    def add_range(self, begin, count, *, group_cull=False, scan_valu=False, job_pixels=0, d_out=None, gamma=True, stream=0):
        """Enqueue the chunks ``[begin, begin + count)`` of every view in one launch; ``d_out``: a device pointer that receives the N
        running images (N*H*W*3 elements, frame after frame)."""
        P = self._params(group_cull, scan_valu, job_pixels, gamma)
        fn = self.L.rtw_render_accum_batch_f64 if _capi.is_f64(self.T) else self.L.rtw_render_accum_batch_f32
        _capi.check(fn(self.handle, self.cams, self.n_views, self.seeds, C.byref(P), int(begin), int(count), self._handles,
                       C.c_void_p(int(d_out)) if d_out else None, C.c_void_p(int(stream))))

    def images(self, gamma=True):
        """The images of the samples added so far (blocking): ``imgs[v, i, j, :]``, view ``v`` like ``render``'s image.  ONE resolve launch
        for all views (``images_into``) and one copy back; view ``v`` is bit for bit ``ProgressiveRenderer.image()``.  Like ``features()``
        it takes its device buffer from torch (RuntimeError without a GPU torch sees; torch must have initialised the GPU first,
        INTEGRATION.md section 5).  An adaptive view whose last ``run`` failed half way is refused (RtwError -2) until a ``run`` finishes."""
        import torch
        buf = self._device_buffer(self.n_views * self.height * self.width * 3)
        self.images_into(buf.data_ptr(), gamma, stream=torch.cuda.current_stream(buf.device).cuda_stream)
        return buf.cpu().numpy().reshape(self.n_views, self.width, self.height, 3).transpose(0, 2, 1, 3)

    def read_pixels(self, v):
        """View ``v``'s accumulator (blocking): ``words[i, j, :]`` as ``ProgressiveRenderer.read_pixels``."""
        out = np.empty(self.height * self.width * 8, dtype=np.uint64)
        _capi.check(self.L.rtw_accum_read_pixels(self.accums[v], out.ctypes.data_as(C.c_void_p)))
        return out.reshape(self.width, self.height, 8).transpose(1, 0, 2)

    def info(self, v):
        st = _capi.AccumInfo()
        _capi.check(self.L.rtw_accum_info(self.accums[v], C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def _filtered(self, v, guided, gamma, kw):
        from .denoise import make_denoise
        D = make_denoise(gamma=gamma, **kw)
        P = self._params(False, False, 0, gamma)
        P.seed = int(self.seeds[v])
        out = np.empty(self.height * self.width * 3, dtype=self.T)
        fn = self.L.rtw_accum_filtered_f64 if _capi.is_f64(self.T) else self.L.rtw_accum_filtered_f32
        _capi.check(fn(self.handle, C.byref(self.cams[v]), C.byref(P), C.byref(D), self.accums[v], 1 if guided else 0, out.ctypes.data_as(C.c_void_p)))
        return _as_image(out, self.height, self.width)

    def denoised(self, v, gamma=True, **params):
        """View ``v``'s image so far, filtered with the features of exactly the samples it holds (``ProgressiveRenderer.denoised``)."""
        return self._filtered(v, False, gamma, params)

    # ---- all views in each launch (rtw_accum_*_batch_*): view v is, bit for bit, the per-view method ----
    def _device_buffer(self, n_elems):
        """a torch tensor on the accumulators' device (``ProgressiveRenderer._device_buffer``)"""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("torch sees no GPU: a host copy of a device-resident result needs torch for its device buffer")
        dev = self.info(0)["device"]
        return torch.empty(int(n_elems), dtype=torch.float64 if _capi.is_f64(self.T) else torch.float32, device=f"cuda:{dev}")

    def _sfx(self):
        return "f64" if _capi.is_f64(self.T) else "f32"

    def images_into(self, d_out_ptr, gamma=True, stream=0):
        """Enqueue ONE resolve launch for all views (rtw_accum_resolve_batch_*) into device memory at ``d_out_ptr``: N*H*W*3 elements,
        view ``v`` at ``v*H*W*3`` in the layout of ``ProgressiveRenderer.image_into``."""
        fn = getattr(self.L, "rtw_accum_resolve_batch_" + self._sfx())
        _capi.check(fn(self._handles, self.n_views, 1 if gamma else 0, C.c_void_p(int(d_out_ptr)), C.c_void_p(int(stream))))

    def features_all_into(self, d_out_ptr, *, scan_valu=False, group_cull=False, job_pixels=0, stream=0):
        """Enqueue ONE feature launch over exactly the samples every view holds (rtw_accum_features_batch_*) into device memory at
        ``d_out_ptr``: N*H*W*8 elements, 16-byte aligned, view ``v`` at ``v*H*W*8``.  Uniform accumulators must all hold the same single
        chunk interval; adaptive ones get, per tile, the features of the chunks ``[0, C_t)`` of their own view."""
        P = self._params(group_cull, scan_valu, job_pixels, True)
        fn = getattr(self.L, "rtw_accum_features_batch_" + self._sfx())
        _capi.check(fn(self.handle, self.cams, self.n_views, self.seeds, C.byref(P), self._handles, C.c_void_p(int(d_out_ptr)), C.c_void_p(int(stream))))

    def features_all(self, **kw):
        """The first-hit features of the samples every view holds (blocking): the dict of ``render_features_batch``, arrays ``[N, H, W, ...]``."""
        import torch
        from .features import FEATURE_CHANNELS, split
        buf = self._device_buffer(self.n_views * self.height * self.width * FEATURE_CHANNELS)
        self.features_all_into(buf.data_ptr(), stream=torch.cuda.current_stream(buf.device).cuda_stream, **kw)
        raw = buf.cpu().numpy()
        return split(raw.reshape(self.n_views, self.width, self.height, FEATURE_CHANNELS).transpose(0, 2, 1, 3))

    def _filtered_all(self, guided, gamma, kw):
        from .denoise import make_denoise
        D = make_denoise(gamma=gamma, **kw)
        P = self._params(False, False, 0, gamma)
        out = np.empty(self.n_views * self.height * self.width * 3, dtype=self.T)
        fn = getattr(self.L, "rtw_accum_filtered_batch_" + self._sfx())
        _capi.check(fn(self.handle, self.cams, self.n_views, self.seeds, C.byref(P), C.byref(D), self._handles, 1 if guided else 0, out.ctypes.data_as(C.c_void_p)))
        return out.reshape(self.n_views, self.width, self.height, 3).transpose(0, 2, 1, 3)

    def denoised_all(self, gamma=True, **params):
        """``denoised(v)`` of every view, ``[N, H, W, 3]``, in 3 + ``levels`` launches and one copy for any N (rtw_accum_filtered_batch_*, blocking)."""
        return self._filtered_all(False, gamma, params)

    def ranges(self, v):
        """the chunk ranges view ``v`` holds: sorted list of ``(begin, end)``, end exclusive"""
        n = C.c_int32(0)
        _capi.check(self.L.rtw_accum_ranges(self.accums[v], 0, C.byref(n), None))
        buf = (C.c_int32 * (2 * max(n.value, 1)))()
        _capi.check(self.L.rtw_accum_ranges(self.accums[v], n.value, C.byref(n), buf))
        return [(int(buf[2 * k]), int(buf[2 * k + 1])) for k in range(n.value)]

    def stats(self):
        """Counters / kernel time of the calling thread's last call (waits for it): the sums over the views."""
        st = _capi.Stats()
        _capi.check(self.L.rtw_stats(C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def close(self):
        for acc in getattr(self, "accums", []):
            if acc:
                self.L.rtw_accum_free(acc)
        self.accums = []
        if getattr(self, "handle", None):
            self.L.rtw_scene_free(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_progressive(scene, cam, image_width=400, n_samples=1, *, passes=4, callback=None, depth=16, seed=1, n_chunks=0, device=-1,
                       gamma=True, group_cull=False, scan_valu=False, numerics=None):
    """``render(...)`` in ``passes`` passes of (nearly) equal chunk counts; the return value equals ``render``'s with the same
    arguments, bit for bit.  ``callback(renderer, samples_done)`` runs after each pass is enqueued (``renderer.image()`` there gives
    the picture so far; a true return value stops the render early, and the image of what was added is returned)."""
    if int(passes) < 1:
        raise ValueError("passes must be >= 1")
    with ProgressiveRenderer(scene, cam, image_width, n_samples, depth=depth, seed=seed, n_chunks=n_chunks, device=device,
                             numerics=numerics) as pr:
        k = min(int(passes), pr.n_chunks)
        for i in range(k):
            begin, end = i * pr.n_chunks // k, (i + 1) * pr.n_chunks // k
            done = pr.add_range(begin, end - begin, group_cull=group_cull, scan_valu=scan_valu)
            if callback is not None and callback(pr, done):
                break
        return pr.image(gamma=gamma)
