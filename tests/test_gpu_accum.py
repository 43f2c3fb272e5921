"""Progressive render on the GPU (include/rtw_hip.h rtw_render_accum_*, rtw_accum_*): any partition of a render's chunks into passes --
in any order, in any mix of scan modes and job sizes, on one accumulator or merged from several, across an export / import -- resolves to
the image of the single rtw_render_* call; every prefix [0, C) is the render with spp = min(S, C * chunk size), n_chunks = C; and the
accumulator holds the exact 64.64 sum of the oracle's per-sample radiances.  Every comparison is on the bits.  Tolerance: NONE."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from conftest import CamObj, load_golden

pytestmark = pytest.mark.gpu

SCANS = {"matrix": 0, "valu": 4, "cull": 1}          # rtw_params.flags: matrix pipe (default), RTW_FLAG_SCAN_VALU, RTW_FLAG_GROUP_CULL


def _image(flat, width, height):
    return flat.reshape(width, height, 3).transpose(1, 0, 2)


def single(flat, cam, T, width, height, spp, depth, seed, n_chunks=0, flags=0, gamma=1):
    """the one-shot rtw_render_* -> (img[i, j, c], stats)"""
    from rtw_amd import _capi
    L = _capi.lib()
    S, keep = _capi.make_scene(flat, T)
    Cm = _capi.make_camera(cam, T)
    P = _capi.make_params(width=width, height=height, spp=spp, max_depth=depth, seed=seed, n_chunks=n_chunks, flags=flags, gamma=gamma)
    out = np.empty(width * height * 3, T)
    fn = L.rtw_render_f64 if T is np.float64 else L.rtw_render_f32
    _capi.check(fn(C.byref(S), C.byref(Cm), C.byref(P), out.ctypes.data_as(C.c_void_p)))
    st = _capi.Stats()
    _capi.check(L.rtw_stats(C.byref(st)))
    return _image(out, width, height), st


class Acc:
    """an uploaded scene + one accumulator, straight on the C ABI (device 0); `add` returns the call's return code"""

    def __init__(self, flat, cam, T, width, height, spp, depth, seed, n_chunks=0, scene_from=None, blob=None):
        from rtw_amd import _capi
        from rtw_amd.progressive import effective_chunks
        self.C, self.L, self.T = _capi, _capi.lib(), T
        self.flat, self.cam, self.width, self.height = flat, cam, width, height
        self.spp, self.depth, self.seed, self.n_chunks_arg = spp, depth, seed, n_chunks
        self.n_chunks, self.chunk_spp = effective_chunks(spp, n_chunks)
        self.owns_scene = scene_from is None
        if scene_from is None:
            S, keep = _capi.make_scene(flat, T)
            self.scene = C.c_void_p()
            _capi.check((self.L.rtw_scene_upload_f64 if T is np.float64 else self.L.rtw_scene_upload_f32)(C.byref(S), 0, C.byref(self.scene)))
        else:
            self.scene = scene_from.scene
        self.acc = C.c_void_p()
        if blob is None:
            _capi.check(self.L.rtw_accum_create(0, width, height, C.byref(self.acc)))
        else:
            _capi.check(self.L.rtw_accum_import(0, blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(self.acc)))

    def add(self, begin, count, flags=0, job_pixels=0, d_out=None, stream=0, gamma=1, cam=None, seed=None, spp=None, depth=None,
            n_chunks=None, width=None, height=None, scene=None):
        P = self.C.make_params(width=width or self.width, height=height or self.height, spp=spp or self.spp,
                               max_depth=self.depth if depth is None else depth, seed=self.seed if seed is None else seed,
                               n_chunks=self.n_chunks_arg if n_chunks is None else n_chunks, flags=flags, gamma=gamma, job_pixels=job_pixels)
        Cm = self.C.make_camera(cam or self.cam, self.T)
        fn = self.L.rtw_render_accum_f64 if self.T is np.float64 else self.L.rtw_render_accum_f32
        return fn(scene or self.scene, C.byref(Cm), C.byref(P), begin, count, self.acc, C.c_void_p(d_out) if d_out else None,
                  C.c_void_p(stream) if stream else None)

    def add_ok(self, *a, **kw):
        self.C.check(self.add(*a, **kw))
        st = self.C.Stats()
        self.C.check(self.L.rtw_stats(C.byref(st)))
        return st

    def resolve(self, gamma=1):
        out = np.empty(self.width * self.height * 3, self.T)
        fn = self.L.rtw_accum_resolve_host_f64 if self.T is np.float64 else self.L.rtw_accum_resolve_host_f32
        self.C.check(fn(self.acc, gamma, out.ctypes.data_as(C.c_void_p)))
        return _image(out, self.width, self.height)

    def words(self):
        out = np.empty(self.width * self.height * 8, np.uint64)
        self.C.check(self.L.rtw_accum_read_pixels(self.acc, out.ctypes.data_as(C.c_void_p)))
        return out.reshape(self.width, self.height, 8).transpose(1, 0, 2)

    def info(self):
        st = self.C.AccumInfo()
        self.C.check(self.L.rtw_accum_info(self.acc, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def export(self):
        size = C.c_uint64()
        self.C.check(self.L.rtw_accum_export(self.acc, None, 0, C.byref(size)))
        buf = np.empty(size.value, np.uint8)
        assert self.L.rtw_accum_export(self.acc, buf.ctypes.data_as(C.c_void_p), size.value - 1, C.byref(size)) == -2      # (too small)
        self.C.check(self.L.rtw_accum_export(self.acc, buf.ctypes.data_as(C.c_void_p), size.value, C.byref(size)))
        return buf

    def merge(self, other, stream=0):
        return self.L.rtw_accum_merge(self.acc, other.acc, C.c_void_p(stream) if stream else None)

    def free_accum(self):
        self.C.check(self.L.rtw_accum_free(self.acc))
        self.acc = C.c_void_p()

    def close(self):
        if self.acc:
            self.free_accum()
        if self.owns_scene and self.scene:
            self.L.rtw_scene_free(self.scene)
            self.scene = C.c_void_p()


def _golden_acc(name, n_chunks=None):
    g = load_golden(name)
    T = g["image"].dtype.type
    a = Acc(g["flat"], CamObj(g["cam"]), T, g["width"], g["height"], g["spp"], g["depth"], g["seed"], g["n_chunks"] if n_chunks is None else n_chunks)
    return g, T, a


def _uneven(n):
    """[0,1) [1,7) [7,n) (fewer for a short render), issued last-first-middle"""
    cuts = sorted({0, min(1, n), min(7, n), n})
    rs = [(b, e - b) for b, e in zip(cuts[:-1], cuts[1:])]
    return rs[-1:] + rs[:1] + rs[1:-1]


def _same(a, b):
    """bitwise equality, NaNs included"""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- 1. partition = single render -------------------------------------------------------------------------------------------------
@pytest.mark.usefixtures("numerics")
@pytest.mark.parametrize("scan", list(SCANS))
@pytest.mark.parametrize("name", ["cfg1_2spheres_96x54_16spp_d4_f32", "random_64x36_8spp_d50_f64", "cfg2_random_320x180_64spp_d16_f32"])
def test_uneven_shuffled_passes_equal_the_golden(name, scan):
    g, T, a = _golden_acc(name)
    try:
        seg = samples = 0
        for b, c in _uneven(a.n_chunks):
            st = a.add_ok(b, c, flags=SCANS[scan])
            seg += st.segments
            samples += st.samples
            assert st.n_chunks == c                                  # (rtw_stats reports the pass alone)
        info = a.info()
        assert info["complete"] == 1 and info["samples_done"] == g["spp"] and info["chunks_done"] == a.n_chunks
        assert _same(a.resolve(), g["image"])
        assert seg == g["segments"] and samples == g["width"] * g["height"] * g["spp"]
    finally:
        a.close()


@pytest.mark.usefixtures("numerics")
@pytest.mark.parametrize("scan", list(SCANS))
def test_chunks_of_several_samples_with_a_short_last_chunk(scan):
    """16 spp in 3 chunks: 6 + 6 + 4 samples"""
    g, T, a = _golden_acc("cfg1_2spheres_96x54_16spp_d4_f32", n_chunks=3)
    try:
        assert (a.n_chunks, a.chunk_spp) == (3, 6)
        ref, st1 = single(g["flat"], a.cam, T, a.width, a.height, 16, a.depth, a.seed, n_chunks=3)
        seg = 0
        for b in (2, 0, 1):
            seg += a.add_ok(b, 1, flags=SCANS[scan]).segments
        assert a.info()["samples_done"] == 16
        assert _same(a.resolve(), ref) and seg == st1.segments
    finally:
        a.close()


# ---- 2. prefix = standalone render ------------------------------------------------------------------------------------------------
@pytest.mark.usefixtures("numerics")
@pytest.mark.parametrize("name,n_chunks", [("cfg1_2spheres_96x54_16spp_d4_f32", 8), ("random_64x36_8spp_d50_f64", 0),
                                           ("cfg1_2spheres_96x54_16spp_d4_f32", 3)])
def test_every_prefix_is_a_render_of_its_own(oracle, name, n_chunks):
    import torch
    g, T, a = _golden_acc(name, n_chunks=n_chunks)
    try:
        d_img = torch.full((a.width * a.height * 3,), -1.0, dtype=torch.float64 if T is np.float64 else torch.float32, device="cuda:0")
        done = 0
        for C_ in sorted({1, min(3, a.n_chunks), a.n_chunks}):
            a.add_ok(done, C_ - done, d_out=d_img.data_ptr())
            done = C_
            spp = min(a.spp, C_ * a.chunk_spp)
            assert a.info()["samples_done"] == spp
            torch.cuda.synchronize()
            running = _image(d_img.cpu().numpy(), a.width, a.height)
            ref, _ = single(g["flat"], a.cam, T, a.width, a.height, spp, a.depth, a.seed, n_chunks=C_)
            assert _same(running, ref), C_
            assert _same(a.resolve(), ref), C_
            oref, _ = oracle.render(g["flat"], g["cam"], a.width, a.height, spp, T=T, max_depth=a.depth, seed=a.seed, n_chunks=C_,
                                    product_order=oracle.PRODUCT_FORWARD)
            assert _same(ref, oref), C_
    finally:
        a.close()


# ---- 3. the accumulator is the exact sum ------------------------------------------------------------------------------------------
def _fx(x):
    """one radiance as the kernel adds it: truncated towards zero at 2^-64, as a Python integer"""
    q = int(abs(Fraction(float(x))) * 2 ** 64)
    return -q if x < 0 else q


def _signed128(lo, hi):
    v = int(lo) | (int(hi) << 64)
    return v - (1 << 128) if v >> 127 else v


@pytest.mark.usefixtures("numerics")
@pytest.mark.parametrize("name", ["random_64x36_8spp_d50_f64", "cfg2_random_320x180_64spp_d16_f32"])
def test_accumulator_words_are_the_exact_sum_of_the_oracle_samples(oracle, name):
    g, T, a = _golden_acc(name)
    try:
        H, W = a.height, a.width
        glass = (H // 2 - H // 12, W // 2)          # the big glass sphere of the random scene stands at the middle of the frame
        pixels = [(1, 1), (H, 1), (1, W), (H, W), (H // 2, W // 2), glass]
        done = 0
        for C_ in (3, a.n_chunks):
            a.add_ok(done, C_ - done)
            done = C_
            n = a.info()["samples_done"]
            words = a.words()
            for (i, j) in pixels:
                s = oracle.pixel_samples(g["flat"], g["cam"], W, H, a.spp, i, j, T=T, max_depth=a.depth, seed=a.seed, n_chunks=a.n_chunks_arg or None)
                w = words[i - 1, j - 1]
                for ch in range(3):
                    assert _signed128(w[2 * ch], w[2 * ch + 1]) == sum(_fx(x) for x in s[:n, ch]), (C_, i, j, ch)
                assert w[6] == 0 and w[7] == 0
    finally:
        a.close()


# ---- 4. scheduling does not matter -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("width,height", [(100, 56), (1, 1), (13, 7)])
@pytest.mark.parametrize("gamma", [1, 0])
def test_scan_modes_job_sizes_ragged_frames(rtw, T, width, height, gamma):
    import torch
    flat = rtw.flatten_scene(rtw.scene_random_spheres(elem_type=T), T)
    cam = rtw.t_cam1(elem_type=T)
    spp = 10
    a = Acc(flat, cam, T, width, height, spp, 16, 5)
    try:
        d_img = torch.full((width * height * 3,), -1.0, dtype=torch.float64 if T is np.float64 else torch.float32, device="cuda:0")
        plan = [(0, 2, "matrix", 0), (2, 1, "valu", 1), (3, 2, "cull", 4), (5, 1, "matrix", 8), (6, 2, "valu", 16), (8, 1, "cull", 1), (9, 1, "matrix", 4)]
        for b, c, scan, jp in plan:
            a.add_ok(b, c, flags=SCANS[scan], job_pixels=jp, d_out=d_img.data_ptr(), gamma=gamma)
        ref, _ = single(flat, cam, T, width, height, spp, 16, 5, gamma=gamma)
        torch.cuda.synchronize()
        assert _same(_image(d_img.cpu().numpy(), width, height), ref)
        assert _same(a.resolve(gamma), ref)
        assert _same(a.resolve(1 - gamma), single(flat, cam, T, width, height, spp, 16, 5, gamma=1 - gamma)[0])
    finally:
        a.close()


# ---- 5. merge ---------------------------------------------------------------------------------------------------------------------
def test_two_streams_two_accumulators_merged(rtw):
    import torch
    g, T, a = _golden_acc("cfg2_random_320x180_64spp_d16_f32")
    b = Acc(g["flat"], a.cam, T, a.width, a.height, a.spp, a.depth, a.seed, a.n_chunks_arg, scene_from=a)
    try:
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        for k in range(0, a.n_chunks, 16):                       # interleaved ranges of 8 chunks, each accumulator on its own stream
            assert a.add(k, 8, stream=sa.cuda_stream) == 0     # (no rtw_stats in between: nothing waits, the two streams overlap)
            assert b.add(k + 8, 8, stream=sb.cuda_stream, flags=SCANS["cull"]) == 0
        assert a.info()["chunks_done"] == 32 and b.info()["samples_done"] == 32
        assert a.merge(b, sa.cuda_stream) == 0                  # (ordered behind b's stream by the library)
        assert a.info()["complete"] == 1
        assert _same(a.resolve(), g["image"])
        # b is left as it was; merging it again overlaps
        before = a.words().copy()
        assert a.merge(b) == -2 and b"both accumulators" in a.L.rtw_last_error()
        assert b.info()["chunks_done"] == 32
        assert np.array_equal(a.words(), before)
    finally:
        b.close()
        a.close()


def test_merge_refuses_other_renders_and_leaves_dst_alone(rtw):
    T = np.float32
    flat = rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T)
    flat2 = rtw.flatten_scene(rtw.scene_4_spheres(elem_type=T), T)
    cam, cam2 = rtw.t_default_cam(elem_type=T), rtw.t_cam2(elem_type=T)
    dst = Acc(flat, cam, T, 96, 54, 8, 8, 1)
    others = {"seed": Acc(flat, cam, T, 96, 54, 8, 8, 2), "camera": Acc(flat, cam2, T, 96, 54, 8, 8, 1),
              "scene": Acc(flat2, cam, T, 96, 54, 8, 8, 1), "spp": Acc(flat, cam, T, 96, 54, 9, 8, 1),
              "size": Acc(flat, cam, T, 64, 36, 8, 8, 1)}
    try:
        dst.add_ok(0, 4)
        before = dst.words().copy()
        for why, o in others.items():
            o.add_ok(4, 4)
            assert dst.merge(o) == -4, why
            assert dst.info()["chunks_done"] == 4
        assert np.array_equal(dst.words(), before)
        # an empty accumulator merges as nothing; into an empty one: the binding travels
        empty = Acc(flat, cam, T, 96, 54, 8, 8, 1, scene_from=dst)
        assert dst.merge(empty) == 0 and np.array_equal(dst.words(), before)
        assert empty.merge(dst) == 0 and np.array_equal(empty.words(), before) and empty.info()["samples_done"] == 4
        empty.add_ok(4, 4)
        assert _same(empty.resolve(), single(flat, cam, T, 96, 54, 8, 8, 1)[0])
        empty.close()
    finally:
        for o in others.values():
            o.close()
        dst.close()


# ---- 6. checkpoint -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg1_2spheres_96x54_16spp_d4_f32", "random_64x36_8spp_d50_f64"])
def test_export_free_import_finish(name):
    g, T, a = _golden_acc(name)
    b = None
    try:
        a.add_ok(2, 3)
        a.add_ok(0, 1)
        info = a.info()
        words = a.words().copy()
        blob = a.export()
        a.free_accum()
        a.L.rtw_shutdown()                                       # (accumulators and blobs do not depend on the library's caches)
        b = Acc(g["flat"], a.cam, T, a.width, a.height, a.spp, a.depth, a.seed, a.n_chunks_arg, scene_from=a, blob=blob)
        assert b.info() == info and np.array_equal(b.words(), words)
        assert b.add(2, 1) == -2                                 # the ranges came along
        assert b.add(1, 1, seed=a.seed + 1) == -4                # ... and the binding
        b.add_ok(1, 1)
        b.add_ok(5, a.n_chunks - 5)
        assert b.info()["complete"] == 1
        assert _same(b.resolve(), g["image"])
        bad = blob.copy()
        bad[8] = 7                                               # another version
        h = C.c_void_p()
        assert a.L.rtw_accum_import(0, bad.ctypes.data_as(C.c_void_p), bad.size, C.byref(h)) == -2 and not h
        assert a.L.rtw_accum_import(0, blob.ctypes.data_as(C.c_void_p), blob.size - 64, C.byref(h)) == -2 and not h
    finally:
        if b is not None:
            b.close()
        a.close()


def test_shutdown_does_not_invalidate_a_live_accumulator():
    g, T, a = _golden_acc("cfg1_2spheres_96x54_16spp_d4_f32")
    try:
        a.add_ok(0, 5)
        assert a.L.rtw_shutdown() == 0
        a.add_ok(5, 11)
        assert _same(a.resolve(), g["image"])
    finally:
        a.close()


# ---- 7. poison travels ------------------------------------------------------------------------------------------------------------
def test_poisoned_pixels_stay_poisoned(rtw, oracle):
    """every albedo 1e12: a path's radiance leaves the 64.64 range after a few bounces -> the pixel's poison count -> NaN"""
    T = np.float32
    flat = rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T)
    for k in ("ar", "ag", "ab"):
        flat[k] = np.full_like(flat[k], 1e12)
    cam = rtw.t_default_cam(elem_type=T)
    ref, _ = single(flat, cam, T, 96, 54, 16, 4, 1)
    oref, _ = oracle.render(flat, cam, 96, 54, 16, T=T, max_depth=4, seed=1, n_chunks=16, product_order=oracle.PRODUCT_FORWARD)
    mask = np.isnan(ref).any(axis=2)
    assert mask.any() and not mask.all() and np.array_equal(mask, np.isnan(oref).any(axis=2))
    a = Acc(flat, cam, T, 96, 54, 16, 4, 1)
    b = Acc(flat, cam, T, 96, 54, 16, 4, 1, scene_from=a)
    try:
        a.add_ok(0, 4)
        early = np.isnan(a.resolve()).any(axis=2)
        assert early.any() and not (early & ~mask).any()
        assert (a.words()[..., 6] > 0)[early].all()
        a.add_ok(4, 5, flags=SCANS["valu"])
        mid = np.isnan(a.resolve()).any(axis=2)
        assert not (early & ~mid).any()
        b.add_ok(9, 7, flags=SCANS["cull"])
        assert a.merge(b) == 0
        img = a.resolve()
        assert _same(img, ref)
        assert np.array_equal(np.isnan(img).any(axis=2), mask) and not (early & ~mask).any()
        assert np.array_equal(img[~mask], ref[~mask])
    finally:
        b.close()
        a.close()


# ---- 8. misuse on a device ---------------------------------------------------------------------------------------------------------
def test_misuse_is_refused_and_leaves_the_words_alone(rtw):
    T = np.float32
    flat = rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T)
    cam, cam2 = rtw.t_default_cam(elem_type=T), rtw.t_cam2(elem_type=T)
    a = Acc(flat, cam, T, 96, 54, 8, 8, 1)
    f64 = Acc(rtw.flatten_scene(rtw.scene_2_spheres(elem_type=np.float64), np.float64), rtw.t_default_cam(elem_type=np.float64), np.float64, 96, 54, 8, 8, 1)
    try:
        h = C.c_void_p()
        out = np.empty(96 * 54 * 3, T)
        assert a.L.rtw_accum_resolve_host_f32(a.acc, 1, out.ctypes.data_as(C.c_void_p)) == -2       # nothing in it yet
        a.add_ok(2, 3)
        before = a.words().copy()
        err = a.L.rtw_last_error
        assert a.add(4, 2) == -2 and b"overlaps" in err()                     # overlapping pass
        assert a.add(0, 3) == -2
        assert a.add(0, 1, seed=2) == -4 and b"another render" in err()       # passes of other renders
        assert a.add(0, 1, cam=cam2) == -4
        assert a.add(0, 1, spp=16) == -4
        assert a.add(0, 1, depth=9) == -4
        assert a.add(0, 1, n_chunks=4) == -4
        assert a.add(0, 1, flags=32) == -4                                    # (RTW_FLAG_NUMERICS_CONTRACT)
        assert a.add(0, 1, width=64, height=36) == -4 and b"96 x 54" in err()  # wrong-size accumulator
        assert a.add(0, 1, scene=f64.scene) == -4 and b"precision" in err()
        assert a.L.rtw_accum_resolve_host_f64(a.acc, 1, np.empty(96 * 54 * 3, np.float64).ctypes.data_as(C.c_void_p)) == -4
        assert a.info()["chunks_done"] == 3 and np.array_equal(a.words(), before)
        # flags that do not change the image, and gamma, may differ from pass to pass
        a.add_ok(0, 2, flags=SCANS["cull"], job_pixels=16, gamma=0)
        # reset: zeroed, unbound -- another camera is accepted
        a.C.check(a.L.rtw_accum_reset(a.acc, None))
        assert a.info()["bound"] == 0 and not a.words().any()
        a.add_ok(0, 8, cam=cam2)
        assert _same(a.resolve(), single(flat, cam2, T, 96, 54, 8, 8, 1)[0])
        del h
    finally:
        f64.close()
        a.close()


# ---- 9. the Python layer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_render_progressive_equals_render(rtw, T):
    scene = rtw.scene_random_spheres(elem_type=T)
    cam = rtw.t_cam1(elem_type=T)
    ref = rtw.render(scene, cam, 64, 12, depth=8, seed=3)
    for k in (1, 2, 5, 12, 40):
        seen = []
        img = rtw.render_progressive(scene, cam, 64, 12, passes=k, depth=8, seed=3, callback=lambda pr, done: seen.append(done))
        assert _same(img, ref), k
        assert seen == sorted(seen) and seen[-1] == 12 and len(seen) == min(k, 12)
    ref5 = rtw.render(scene, cam, 64, 12, depth=8, seed=3, n_chunks=5)          # chunks of 3 samples: 4 effective chunks
    assert _same(rtw.render_progressive(scene, cam, 64, 12, passes=3, depth=8, seed=3, n_chunks=5, group_cull=True), ref5)
    # a callback that returns True stops the render: the image of the prefix
    part = rtw.render_progressive(scene, cam, 64, 12, passes=4, depth=8, seed=3, callback=lambda pr, done: done >= 6)
    assert _same(part, rtw.render(scene, cam, 64, 6, depth=8, seed=3))


def test_progressive_renderer_add_merge_save_load(rtw, tmp_path):
    T = np.float32
    scene = rtw.scene_random_spheres(elem_type=T)
    cam = rtw.t_cam1(elem_type=T)
    ref = rtw.render(scene, cam, 64, 10, depth=8, seed=3)
    pr = rtw.ProgressiveRenderer(scene, cam, 64, 10, depth=8, seed=3, device=0)
    assert not pr.done and pr.samples_done == 0 and pr.n_chunks == 10
    assert pr.add() == 1 and pr.add(2, scan_valu=True) == 3
    assert pr.add_range(6, 2, group_cull=True, job_pixels=1) == 5
    assert pr.ranges() == [(0, 3), (6, 8)]
    assert pr.add(100) == 8 and pr.ranges() == [(0, 8)]                       # (up to the chunks already there)
    assert pr.stats()["samples"] == 64 * 36 * 3                                # (the last pass alone)
    assert _same(pr.image(), rtw.render(scene, cam, 64, 8, depth=8, seed=3))
    path = str(tmp_path / "render.rtwacc")
    pr.save(path)
    info = pr.info()
    pr.close()
    pr = rtw.ProgressiveRenderer.load(path, scene, cam)
    assert pr.info() == info and pr.ranges() == [(0, 8)] and (pr.n_samples, pr.depth, pr.seed) == (10, 8, 3)
    other = rtw.ProgressiveRenderer(scene, cam, 64, 10, depth=8, seed=3, device=0)
    other.add_range(8, 2)
    pr.merge(other)
    assert pr.done and pr.samples_done == 10
    with pytest.raises(ValueError):
        pr.add()
    assert _same(pr.image(), ref)
    assert _same(pr.image(gamma=False), rtw.render(scene, cam, 64, 10, depth=8, seed=3, gamma=False))
    import torch
    d = torch.empty(64 * 36 * 3, dtype=torch.float32, device="cuda:0")
    pr.resolve_into(d.data_ptr())
    torch.cuda.synchronize()
    assert _same(_image(d.cpu().numpy(), 64, 36), ref)
    w = pr.read_pixels()
    assert w.shape == (36, 64, 8) and not w[..., 7].any()
    from rtw_amd._capi import RtwError
    with pytest.raises(RtwError) as e:
        other.add_range(8, 1)
    assert e.value.code == -2
    cam2 = rtw.t_cam2(elem_type=T)
    pr.reset(cam2)
    assert pr.samples_done == 0
    pr.add(10)
    assert _same(pr.image(), rtw.render(scene, cam2, 64, 10, depth=8, seed=3))
    with open(path, "rb") as f:
        data = f.read()
    with open(path, "wb") as f:
        f.write(data[:-10])
    with pytest.raises(RtwError) as e:
        rtw.ProgressiveRenderer.load(path, scene, cam)
    assert e.value.code == -2
    other.close()
    pr.close()
