"""The feature-guided upsampler on the GPU (include/rtw_hip.h rtw_upsample_*) against the witness tests/upsample_ref.py.  Every comparison
is on the BITS; NaN pixels are compared as a set.  Tolerance: NONE.
Frames, small (w x h) -> full (W x H): 1x1 -> 1x1 (smallest), 1x1 -> 4x3 (every tap but one outside the frame), 5x3 -> 10x6 (exact 2x),
5x3 -> 11x7 (ragged), 18x10 -> 37x23 (ragged, larger), 35x20 -> 70x41 (several workgroups, one wave in two columns), 70x41 -> 70x41
(ratio 1), 9x40 -> 10x300 (a workgroup inside one column, every fy).  tests/test_upsample_ref.py shows that the committed seeds reach the
spatial fallback, both kinds of NaN pixel and a subnormal sum_w in each of the four larger pairs."""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_ref as DR
import upsample_ref as UR

pytestmark = pytest.mark.gpu

PAIRS = UR.PAIRS
_DEFAULT = dict(levels=2, m=1, demodulate=True, gamma=1, sigma_color=0.5, sigma_depth=0.1, sigma_albedo=0.2)


@functools.lru_cache(maxsize=None)
def _pair(lo, hi, T, seed=None):
    (w, h), (W, H) = lo, hi
    pair = UR.handmade_pair(h, w, H, W, T, UR.SEEDS[T] if seed is None else seed)
    for a in pair:
        a.setflags(write=False)
    return pair


@functools.lru_cache(maxsize=None)
def _witness(lo, hi, T, levels, m, demodulate, gamma, seed=None):
    out = UR.upsample(*_pair(lo, hi, T, seed), T, levels=levels, m=m, demodulate=demodulate, gamma=gamma)
    out.setflags(write=False)
    return out


def _lib_layout(a):
    """[..., rows, cols, c] -> the library's memory: pixel (i, j) at j*rows + i"""
    return np.array(np.swapaxes(a, -3, -2), order="C", copy=True)


def _params(**kw):
    from rtw_amd import _capi
    v = dict(_DEFAULT)
    v.update(kw)
    return _capi.Upsample(v["levels"], v["m"], 1 if v["demodulate"] else 0, v["gamma"], -1, 0, v["sigma_color"], v["sigma_depth"], v["sigma_albedo"])


def upsample_host(image_lo, feat_lo, feat_hi, T, **kw):
    """rtw_upsample_* on [h, w, .] / [H, W, 8] arrays, or rtw_upsample_batch_* on [N, ...] ones -> the result in the inputs' shape"""
    from rtw_amd import _capi
    L = _capi.lib()
    batch = image_lo.ndim == 4
    h, w = image_lo.shape[-3:-1]
    H, W = feat_hi.shape[-3:-1]
    img, flo, fhi = _lib_layout(image_lo), _lib_layout(feat_lo), _lib_layout(feat_hi)
    out = np.full(fhi.shape[:-1] + (3,), -7.0, T)
    U = _params(**kw)
    sfx = "f64" if T is np.float64 else "f32"
    fn = getattr(L, ("rtw_upsample_batch_" if batch else "rtw_upsample_") + sfx)
    views = (image_lo.shape[0],) if batch else ()
    _capi.check(fn(C.byref(U), w, h, W, H, *views, *(a.ctypes.data_as(C.c_void_p) for a in (img, flo, fhi, out))))
    return np.swapaxes(out, -3, -2)


class DevicePair:
    """a pair's inputs (or a batch of pairs, [N, ...]) as torch tensors on cuda:0, and the device entry point on them"""

    def __init__(self, image_lo, feat_lo, feat_hi, T):
        import torch
        from rtw_amd import _capi
        self.L, self.T = _capi.lib(), T
        self.n = image_lo.shape[0] if image_lo.ndim == 4 else 0
        self.h, self.w = image_lo.shape[-3:-1]
        self.H, self.W = feat_hi.shape[-3:-1]
        self.host = [_lib_layout(a) for a in (image_lo, feat_lo, feat_hi)]
        self.img, self.flo, self.fhi = (torch.from_numpy(a).to("cuda:0") for a in self.host)
        self.work_bytes = max(self.n, 1) * int(self.L.rtw_upsample_work_bytes(self.w, self.h, np.dtype(T).itemsize))
        torch.cuda.synchronize()

    def workspace(self, poison=False):
        import torch
        w = torch.zeros(self.work_bytes // np.dtype(self.T).itemsize, dtype=self.img.dtype, device="cuda:0")
        if poison:
            w.fill_(float("nan"))
        return w

    def run(self, work=None, stream=None, **kw):
        """-> the output tensor (not synchronised when a stream is given)"""
        import torch
        from rtw_amd import _capi
        work = self.workspace() if work is None else work
        out = torch.full((max(self.n, 1) * self.W * self.H * 3,), -7.0, dtype=self.img.dtype, device="cuda:0")
        torch.cuda.synchronize()                                   # the fills above ran on torch's stream
        U = _params(**kw)
        sfx = "f64" if self.T is np.float64 else "f32"
        fn = getattr(self.L, ("rtw_upsample_batch_device_" if self.n else "rtw_upsample_device_") + sfx)
        views = (self.n,) if self.n else ()
        _capi.check(fn(C.byref(U), self.w, self.h, self.W, self.H, *views, C.c_void_p(self.img.data_ptr()), C.c_void_p(self.flo.data_ptr()),
                       C.c_void_p(self.fhi.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr()),
                       C.c_void_p(stream.cuda_stream) if stream is not None else None))
        self._keep = work
        if stream is None:
            torch.cuda.synchronize()
        return out

    def image(self, out):
        a = out.cpu().numpy()
        if self.n:
            return a.reshape(self.n, self.W, self.H, 3).transpose(0, 2, 1, 3)
        return a.reshape(self.W, self.H, 3).transpose(1, 0, 2)

    def inputs_unchanged(self):
        return all(np.array_equal(DR.bits(t.cpu().numpy()), DR.bits(a)) for t, a in zip((self.img, self.flo, self.fhi), self.host))


def _assert_same(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: the NaN sets differ ({int(gn.sum())} vs {int(rn.sum())} values)"
    assert np.array_equal(gn.any(axis=-1), gn.all(axis=-1)), f"{what}: a pixel is NaN in some channels only"
    bad = (DR.bits(got) != DR.bits(ref)) & ~gn
    if bad.any():
        where = np.argwhere(bad)[:5]
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} values differ; first index: {where.tolist()}; "
                    f"got {[got[tuple(w)] for w in where]} expected {[ref[tuple(w)] for w in where]}")


# ---- 1. every frame, precision and parameter set through both entry points -------------------------------------------------------------
@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("lo,hi", PAIRS)
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_frames_equal_the_witness(T, lo, hi, entry):
    pair = _pair(lo, hi, T)
    dev = DevicePair(*pair, T) if entry == "device" else None
    work = dev.workspace() if dev else None
    seen_nan = seen_finite = False
    for levels in (0, 2):
        for m in (0, 1, 7):
            for demodulate in (True, False):
                for gamma in (0, 1):
                    kw = dict(levels=levels, m=m, demodulate=demodulate, gamma=gamma)
                    ref = _witness(lo, hi, T, levels, m, demodulate, gamma)
                    got = dev.image(dev.run(work=work, **kw)) if dev else upsample_host(*pair, T, **kw)
                    _assert_same(got, ref, f"{np.dtype(T).name} {lo}->{hi} {entry} {kw}")
                    seen_nan, seen_finite = seen_nan or bool(np.isnan(ref).any()), seen_finite or bool(np.isfinite(ref).any())
    assert seen_finite and (seen_nan or hi[0] * hi[1] < 37 * 23)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_sigmas_reach_the_kernels(T):
    lo, hi = (18, 10), (37, 23)
    pair = _pair(lo, hi, T)
    dev = DevicePair(*pair, T)
    for kw in (dict(sigma_color=0.125), dict(sigma_depth=2.0), dict(sigma_albedo=3.0), dict(sigma_color=3.0, sigma_depth=0.01, sigma_albedo=0.05)):
        ref = UR.upsample(*pair, T, **kw)
        assert not UR.same_bits(ref, _witness(lo, hi, T, 2, 1, True, 1)), kw
        _assert_same(dev.image(dev.run(**kw)), ref, f"device {kw}")
        _assert_same(upsample_host(*pair, T, **kw), ref, f"host {kw}")


# ---- 2. the workspace: poison changes nothing; two streams with a workspace each; the inputs stay ---------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_poisoned_workspace_changes_nothing(T):
    lo, hi = (18, 10), (37, 23)
    dev = DevicePair(*_pair(lo, hi, T), T)
    for levels in (0, 1, 2):
        got = dev.image(dev.run(work=dev.workspace(poison=True), levels=levels))
        ref = UR.upsample(*_pair(lo, hi, T), T, levels=levels)
        _assert_same(got, ref, f"poisoned workspace, levels={levels}")
    assert dev.inputs_unchanged()


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_two_streams_with_separate_workspaces(T):
    import torch
    lo, hi = (35, 20), (70, 41)
    dev = DevicePair(*_pair(lo, hi, T), T)
    ref = _witness(lo, hi, T, 2, 1, True, 1)
    wa, wb = dev.workspace(), dev.workspace(poison=True)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    oa = dev.run(work=wa, stream=sa)
    ob = dev.run(work=wb, stream=sb)
    sa.synchronize()
    sb.synchronize()
    _assert_same(dev.image(oa), ref, "stream a")
    _assert_same(dev.image(ob), ref, "stream b")
    assert dev.inputs_unchanged()


# ---- 3. a batch: view v is the single call ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_batch_equals_its_single_calls(T):
    lo, hi = (18, 10), (37, 23)
    seeds = (31, 32, 33)
    pairs = [_pair(lo, hi, T, s) for s in seeds]
    stacked = [np.stack([p[k] for p in pairs]) for k in range(3)]
    dev = DevicePair(*stacked, T)
    for kw in (dict(), dict(levels=0, m=7, demodulate=False, gamma=0)):
        got_dev = dev.image(dev.run(work=dev.workspace(poison=True), **kw))
        got_host = upsample_host(*stacked, T, **kw)
        for v, s in enumerate(seeds):
            single = upsample_host(*pairs[v], T, **kw)
            _assert_same(single, UR.upsample(*pairs[v], T, **kw), f"single call, view {v} {kw}")
            _assert_same(got_dev[v], single, f"device batch, view {v} {kw}")
            _assert_same(got_host[v], single, f"host batch, view {v} {kw}")
    assert not UR.same_bits(got_host[0], got_host[1])
    assert dev.inputs_unchanged()


# ---- 4. one call equals its parts ----------------------------------------------------------------------------------------------------------
_STAT_KEYS = ("samples", "segments", "sphere_tests", "n_chunks", "grid_blocks", "block_threads")


@pytest.mark.parametrize("group_cull", [False, True])
@pytest.mark.parametrize("scene_name", ["scene_2_spheres", "scene_diel_spheres"])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_render_upsampled_equals_its_parts(rtw, T, scene_name, group_cull):
    """48x27 -> 96x54 at 8 spp: the one call against render (gamma 0) + both feature passes + upsample, and against the witness"""
    scene, cam = getattr(rtw, scene_name)(elem_type=T), rtw.t_default_cam(elem_type=T)
    common = dict(seed=5, group_cull=group_cull)
    lin = rtw.render(scene, cam, 48, 8, gamma=False, **common)
    small_stats = {k: rtw.last_stats()[k] for k in _STAT_KEYS}
    assert lin.shape == (27, 48, 3) and small_stats["samples"] == 48 * 27 * 8
    f_lo = rtw.render_features(scene, cam, 48, 8, seed=5)["raw"]
    for hi_chunks, kw in ((0, dict()), (1, dict(levels=0, normal_power_log2=3, demodulate=False, sigma_albedo=0.5))):
        f_hi = rtw.render_features(scene, cam, 96, 8, seed=5, chunks=None if hi_chunks == 0 else (0, hi_chunks))["raw"]
        for gamma in (True, False):
            got = rtw.render_upsampled(scene, cam, 96, 8, lo_width=48, hi_chunks=hi_chunks, gamma=gamma, **common, **kw)
            assert got.shape == (54, 96, 3) and got.dtype == T
            assert {k: rtw.last_stats()[k] for k in _STAT_KEYS} == small_stats          # rtw_stats: the small render's record
            parts = rtw.upsample(lin, f_lo, f_hi, gamma=gamma, **kw)
            _assert_same(got, parts, f"one call vs its parts, hi_chunks={hi_chunks} gamma={gamma}")
            wkw = dict(levels=kw.get("levels", 2), m=kw.get("normal_power_log2", 1), demodulate=kw.get("demodulate", True),
                       sigma_albedo=kw.get("sigma_albedo", 0.2), gamma=int(gamma))
            ref = UR.upsample(np.ascontiguousarray(lin), np.ascontiguousarray(f_lo), np.ascontiguousarray(f_hi), T, **wkw)
            _assert_same(got, ref, f"one call vs the witness, hi_chunks={hi_chunks} gamma={gamma}")
            assert np.isfinite(got).all()
    # the batched call: 3 cameras, view v is the single call
    cams = [rtw.t_default_cam(elem_type=T), rtw.t_cam1(elem_type=T), rtw.t_cam2(elem_type=T)]
    seeds = [5, 6, 7]
    batch = rtw.render_upsampled_batch(scene, cams, 96, 8, seeds=seeds, lo_width=48, hi_chunks=1, **{k: v for k, v in common.items() if k != "seed"})
    assert batch.shape == (3, 54, 96, 3)
    st = rtw.last_stats()
    assert st["samples"] == 3 * small_stats["samples"] and st["n_chunks"] == small_stats["n_chunks"]
    for v in range(3):
        single = rtw.render_upsampled(scene, cams[v], 96, 8, seed=seeds[v], lo_width=48, hi_chunks=1, group_cull=group_cull)
        _assert_same(batch[v], single, f"batched call, view {v}")
    assert not UR.same_bits(batch[0], batch[1])


def test_stats_still_report_the_previous_render(rtw):
    T = np.float32
    scene, cam = rtw.scene_2_spheres(elem_type=T), rtw.t_default_cam(elem_type=T)
    rtw.render(scene, cam, 96, 4, depth=16, seed=1, device=0)
    from rtw_amd import _capi
    L = _capi.lib()
    before = _capi.Stats()
    _capi.check(L.rtw_stats(C.byref(before)))
    pair = _pair((18, 10), (37, 23), T)
    DevicePair(*pair, T).run()
    upsample_host(*pair, T)
    after = _capi.Stats()
    _capi.check(L.rtw_stats(C.byref(after)))
    for k, _ in _capi.Stats._fields_:
        assert getattr(before, k) == getattr(after, k), k
    assert after.samples == 96 * 54 * 4


def test_python_layer(rtw):
    import torch
    T = np.float32
    lo, hi = (18, 10), (37, 23)
    pair = _pair(lo, hi, T)
    ref = _witness(lo, hi, T, 2, 1, True, 1)
    from rtw_amd.features import split
    _assert_same(rtw.upsample(*pair), ref, "upsample")
    _assert_same(rtw.upsample(pair[0], split(pair[1]), split(pair[2])), ref, "upsample with the dicts of render_features")
    _assert_same(rtw.upsample(*pair, levels=0, normal_power_log2=7, demodulate=False, gamma=False), _witness(lo, hi, T, 0, 7, False, 0), "upsample keywords")
    stacked = [np.stack([a, a]) for a in pair]
    _assert_same(rtw.upsample_batch(*stacked)[1], ref, "upsample_batch")
    dev = DevicePair(*pair, T)
    work, out = dev.workspace(), torch.zeros(37 * 23 * 3, dtype=torch.float32, device="cuda:0")
    assert rtw.upsample_work_bytes(18, 10, T) == dev.work_bytes
    torch.cuda.synchronize()
    rtw.upsample_into(out.data_ptr(), dev.img.data_ptr(), dev.flo.data_ptr(), dev.fhi.data_ptr(), work.data_ptr(), 18, 10, 37, 23, elem_type=T,
                      work_bytes=dev.work_bytes)
    torch.cuda.synchronize()
    _assert_same(dev.image(out), ref, "upsample_into")
    bdev = DevicePair(*stacked, T)
    bwork, bout = bdev.workspace(), torch.zeros(2 * 37 * 23 * 3, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rtw.upsample_batch_into(bout.data_ptr(), bdev.img.data_ptr(), bdev.flo.data_ptr(), bdev.fhi.data_ptr(), bwork.data_ptr(), 18, 10, 37, 23, 2,
                            elem_type=T, work_bytes=bdev.work_bytes)
    torch.cuda.synchronize()
    _assert_same(bdev.image(bout)[0], ref, "upsample_batch_into")
    # the default small frame: ceil(W / 2) wide
    scene, cam = rtw.scene_2_spheres(elem_type=T), rtw.t_default_cam(elem_type=T)
    got = rtw.render_upsampled(scene, cam, 97, 4, seed=3)
    assert got.shape == (54, 97, 3) and rtw.last_stats()["samples"] == 49 * 27 * 4


# ---- 5. it helps: against a plain bilinear resize of the same small image ---------------------------------------------------------------------
def bilinear(image_lo, H, W):
    """[h, w, 3] -> [H, W, 3], pixel centres aligned, edge pixels repeated; binary64"""
    a = np.asarray(image_lo, np.float64)
    h, w = a.shape[:2]

    def axis(small, full):
        pos = np.clip((np.arange(full) + 0.5) * small / full - 0.5, 0, small - 1)
        k = np.minimum(np.floor(pos).astype(int), max(small - 2, 0))
        return k, np.minimum(k + 1, small - 1), pos - k

    i0, i1, fi = axis(h, H)
    j0, j1, fj = axis(w, W)
    rows = a[i0] * (1 - fi)[:, None, None] + a[i1] * fi[:, None, None]
    return rows[:, j0] * (1 - fj)[None, :, None] + rows[:, j1] * fj[None, :, None]


def edge_band(coverage, radius=2):
    """the pixels within `radius` pixels of one with 0 < coverage < 1"""
    edge = (coverage > 0) & (coverage < 1)
    H, W = edge.shape
    band = np.zeros_like(edge)
    for di in range(-radius, radius + 1):
        for dj in range(-radius, radius + 1):
            band[max(0, di):H + min(0, di), max(0, dj):W + min(0, dj)] |= edge[max(0, -di):H + min(0, -di), max(0, -dj):W + min(0, -dj)]
    return band


def test_the_bilinear_yardstick_reproduces_a_plane():
    """(the yardstick itself: a linear ramp sampled at the small centres comes back exactly at the inner full-size centres)"""
    h, w, H, W = 5, 7, 10, 14
    ramp = lambda n, full: ((np.arange(n) + 0.5) * full / n)
    lo = (ramp(h, H)[:, None, None] + 3 * ramp(w, W)[None, :, None]) * np.ones(3)
    hi = ramp(H, H)[:, None, None] + 3 * ramp(W, W)[None, :, None] * np.ones(3)
    got = bilinear(lo, H, W)
    assert np.allclose(got[1:-1, 1:-1], hi[1:-1, 1:-1], rtol=0, atol=1e-12)


@pytest.mark.parametrize("scene_name,cam_name", [("scene_2_spheres", "t_default_cam"), ("scene_random_spheres", "t_cam1")])
def test_it_beats_a_bilinear_resize(rtw, scene_name, cam_name):
    """96x54 -> 192x108 at 8 spp, linear, Float32, default parameters: the RMSE against a 1024-spp render at 192x108, over all pixels and over
    the band within 2 pixels of a partly covered pixel, must be strictly below that of a numpy bilinear resize of the same small image.
    The yardstick is the bilinear image, not the code under test; no ratio is fixed.  Measured."""
    T = np.float32
    scene, cam = getattr(rtw, scene_name)(elem_type=T), getattr(rtw, cam_name)(elem_type=T)
    truth = rtw.render(scene, cam, 192, 1024, seed=99, gamma=False).astype(np.float64)
    small = rtw.render(scene, cam, 96, 8, seed=1, gamma=False)
    up = rtw.render_upsampled(scene, cam, 192, 8, seed=1, gamma=False).astype(np.float64)
    cov = rtw.render_features(scene, cam, 192, 8, seed=1)["coverage"]
    assert truth.shape == up.shape == (108, 192, 3) and small.shape == (54, 96, 3) and np.isfinite(up).all()
    bil = bilinear(small, 108, 192)
    band = edge_band(cov)
    assert 0 < band.sum() < band.size
    rmse = lambda a, mask: float(np.sqrt(np.mean((a[mask] - truth[mask]) ** 2)))
    everything = np.ones_like(band)
    up_all, bil_all, up_band, bil_band = rmse(up, everything), rmse(bil, everything), rmse(up, band), rmse(bil, band)
    print(f"{scene_name}: RMSE all pixels upsampled {up_all:.5f} bilinear {bil_all:.5f} (ratio {up_all / bil_all:.3f}); "
          f"edge band ({int(band.sum())} pixels) upsampled {up_band:.5f} bilinear {bil_band:.5f} (ratio {up_band / bil_band:.3f})")
    assert up_all < bil_all, (up_all, bil_all)
    assert up_band < bil_band, (up_band, bil_band)
