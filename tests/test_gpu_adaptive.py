"""Adaptive sampling on the GPU (include/rtw_hip.h rtw_render_adaptive_*): every 8x8 tile holds a prefix [0, C_t) of the render's chunks,
C_t = the first checkpoint at which the tile passes the stopping rule.  Checked here: an unreachable tolerance is the one-shot render;
word 7 of every pixel is the half difference of the oracle's samples; the C_t are the ones the rule gives on the ORACLE's samples, for a
tolerance picked from those samples so that tiles stop at the first checkpoint, in between and never; every tile is the prefix render of
its C_t; nothing depends on scan mode or job size; refinement equals a fresh run; the bookkeeping adds up.  Every comparison is on the
bits.  Tolerance of the comparisons: NONE."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import CamObj, load_golden

pytestmark = pytest.mark.gpu

SCANS = {"matrix": 0, "valu": 4, "cull": 1}          # rtw_params.flags: matrix pipe (default), RTW_FLAG_SCAN_VALU, RTW_FLAG_GROUP_CULL
FLOOR = 0.03
UNREACHABLE = 1e-300


def _image(flat, width, height):
    return flat.reshape(width, height, 3).transpose(1, 0, 2)


def _same(a, b):
    """bitwise equality, NaNs included"""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def single(flat, cam, T, width, height, spp, depth, seed, n_chunks=0, flags=0, gamma=1):
    """the one-shot rtw_render_* -> img[i, j, c]"""
    from rtw_amd import _capi
    L = _capi.lib()
    S, keep = _capi.make_scene(flat, T)
    Cm = _capi.make_camera(cam, T)
    P = _capi.make_params(width=width, height=height, spp=spp, max_depth=depth, seed=seed, n_chunks=n_chunks, flags=flags, gamma=gamma)
    out = np.empty(width * height * 3, T)
    fn = L.rtw_render_f64 if T is np.float64 else L.rtw_render_f32
    _capi.check(fn(C.byref(S), C.byref(Cm), C.byref(P), out.ctypes.data_as(C.c_void_p)))
    return _image(out, width, height)


class Ad:
    """an uploaded scene + one accumulator, straight on the C ABI (device 0)"""

    def __init__(self, flat, cam, T, width, height, spp, depth, seed, n_chunks=0, floor=FLOOR, min_chunks=0, check_chunks=0):
        from rtw_amd import _capi
        from rtw_amd.progressive import effective_chunks
        self.C, self.L, self.T = _capi, _capi.lib(), T
        self.flat, self.cam, self.width, self.height = flat, cam, width, height
        self.spp, self.depth, self.seed, self.n_chunks_arg = spp, depth, seed, n_chunks
        self.floor, self.min_chunks, self.check_chunks = floor, min_chunks, check_chunks
        self.n_chunks, self.chunk_spp = effective_chunks(spp, n_chunks)
        self.tiles_i, self.tiles_j = (height + 7) // 8, (width + 7) // 8
        S, keep = _capi.make_scene(flat, T)
        self.scene, self.acc = C.c_void_p(), C.c_void_p()
        _capi.check((self.L.rtw_scene_upload_f64 if T is np.float64 else self.L.rtw_scene_upload_f32)(C.byref(S), 0, C.byref(self.scene)))
        _capi.check(self.L.rtw_accum_create(0, width, height, C.byref(self.acc)))

    def _params(self, flags=0, job_pixels=0, gamma=1, seed=None):
        return self.C.make_params(width=self.width, height=self.height, spp=self.spp, max_depth=self.depth, seed=self.seed if seed is None else seed,
                                  n_chunks=self.n_chunks_arg, flags=flags, gamma=gamma, job_pixels=job_pixels)

    def run(self, tol, flags=0, job_pixels=0, d_out=None, gamma=1, floor=None, min_chunks=None, check_chunks=None, seed=None):
        """rtw_render_adaptive_* -> return code"""
        P = self._params(flags, job_pixels, gamma, seed)
        A = self.C.Adaptive(tol, self.floor if floor is None else floor, self.min_chunks if min_chunks is None else min_chunks,
                            self.check_chunks if check_chunks is None else check_chunks)
        Cm = self.C.make_camera(self.cam, self.T)
        fn = self.L.rtw_render_adaptive_f64 if self.T is np.float64 else self.L.rtw_render_adaptive_f32
        return fn(self.scene, C.byref(Cm), C.byref(P), C.byref(A), self.acc, C.c_void_p(d_out) if d_out else None, None)

    def run_ok(self, *a, **kw):
        self.C.check(self.run(*a, **kw))
        return self

    def add(self, begin, count):
        """a plain rtw_render_accum_* pass -> return code"""
        P = self._params()
        Cm = self.C.make_camera(self.cam, self.T)
        fn = self.L.rtw_render_accum_f64 if self.T is np.float64 else self.L.rtw_render_accum_f32
        return fn(self.scene, C.byref(Cm), C.byref(P), begin, count, self.acc, None, None)

    def stats(self):
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

    def chunks(self):
        """C_t in tile order t = tj * tiles_i + ti"""
        n = C.c_int32()
        buf = np.full(self.tiles_i * self.tiles_j, -1, np.int32)
        self.C.check(self.L.rtw_accum_tile_chunks(self.acc, buf.size, C.byref(n), buf.ctypes.data_as(C.POINTER(C.c_int32))))
        assert n.value == buf.size
        return buf

    def info(self):
        st = self.C.AccumInfo()
        self.C.check(self.L.rtw_accum_info(self.acc, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def ainfo(self):
        st = self.C.AdaptiveInfo()
        self.C.check(self.L.rtw_accum_adaptive_info(self.acc, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def ranges(self):
        n = C.c_int32()
        buf = (C.c_int32 * 8)()
        self.C.check(self.L.rtw_accum_ranges(self.acc, 4, C.byref(n), buf))
        return [(buf[2 * k], buf[2 * k + 1]) for k in range(n.value)]

    def tile_mask(self, t):
        """bool H x W: the pixels of tile t"""
        tj, ti = divmod(int(t), self.tiles_i)
        m = np.zeros((self.height, self.width), bool)
        m[ti * 8:ti * 8 + 8, tj * 8:tj * 8 + 8] = True
        return m

    def npix(self, t):
        return int(self.tile_mask(t).sum())

    def close(self):
        if self.acc:
            self.L.rtw_accum_free(self.acc)
            self.acc = C.c_void_p()
        if self.scene:
            self.L.rtw_scene_free(self.scene)
            self.scene = C.c_void_p()


# ---- the oracle's side: samples -> accumulator words, in Python integers ------------------------------------------------------------
def _fx(x):
    """one radiance as the kernel adds it (64.64, truncated towards zero) as a Python integer; None: it poisons the pixel"""
    x = float(x)
    if not (abs(x) < 2147483648.0):
        return None
    m, e = math.frexp(abs(x))
    mant, sh = int(m * 2 ** 53), e - 53 + 64
    v = mant << sh if sh >= 0 else mant >> -sh
    return -v if x < 0 else v


def _q(fx):
    return 0 if fx is None or fx < 0 else min(fx >> 40, 2 ** 30 - 1)


def oracle_words(samples, chunk_spp, counts):
    """samples[i, j, k, c] (float64: every sample of every pixel, in sample order) -> {n: words[i, j, 8] after the first n samples}
    for the sample counts `counts`: the 128-bit sums, the poison count and the half difference H_p"""
    H, W, S, _ = samples.shape
    out = {n: np.zeros((H, W, 8), np.uint64) for n in counts}
    M64 = (1 << 64) - 1
    for i in range(H):
        for j in range(W):
            sums, poison, h = [0, 0, 0], 0, 0
            for k in range(S):
                odd = (k // chunk_spp) & 1
                for c in range(3):
                    fx = _fx(samples[i, j, k, c])
                    if fx is None:
                        poison += 1
                    else:
                        sums[c] += fx
                        h += -_q(fx) if odd else _q(fx)
                if k + 1 in out:
                    w = out[k + 1][i, j]
                    for c in range(3):
                        v = sums[c] & ((1 << 128) - 1)
                        w[2 * c], w[2 * c + 1] = v & M64, v >> 64
                    w[6], w[7] = poison, h & M64
    return out


def all_samples(oracle, flat, cam, T, width, height, spp, depth, seed, n_chunks):
    out = np.empty((height, width, spp, 3), np.float64)
    for i in range(height):
        for j in range(width):
            out[i, j] = oracle.pixel_samples(flat, cam, width, height, spp, i + 1, j + 1, T=T, max_depth=depth, seed=seed, n_chunks=n_chunks)
    return out


def rule_chunks(words_at, checkpoints, n_chunks, chunk_spp, width, height, tol, floor):
    """C_t by the written rule (rtw_amd.reference_decisions) from {c: words after the chunks [0, c)}"""
    from rtw_amd import reference_decisions
    n_tiles = ((height + 7) // 8) * ((width + 7) // 8)
    ct = np.full(n_tiles, n_chunks, np.int32)
    for c in reversed(checkpoints):
        conv = reference_decisions(words_at[c], width, height, c * chunk_spp, tol, floor)
        ct[conv] = c
    return ct


# ---- the shared case: cfg2's scene and camera at 48 x 27 (6 x 4 tiles, a ragged last row), 64 chunks of one sample ----------------
W48, H27, SPP, DEPTH, SEED = 48, 27, 64, 8, 7
CHECKS = [16, 32, 48]


@pytest.fixture(scope="module")
def case48(oracle):
    """oracle samples of every pixel, the words they give at every checkpoint, the ratios D / M of every tile there, and a tolerance
    picked from those ratios (conditions (a) - (d) below are asserted by the decision test)"""
    from rtw_amd import reference_decisions
    g = load_golden("cfg2_random_320x180_64spp_d16_f32", numerics="reference")
    T = np.float32
    cam = CamObj(g["cam"])
    samples = all_samples(oracle, g["flat"], g["cam"], T, W48, H27, SPP, DEPTH, SEED, SPP)
    words_at = oracle_words(samples, 1, CHECKS + [SPP])
    ratios = {}
    for c in CHECKS:
        _, D, Y, M = reference_decisions(words_at[c], W48, H27, c, 1.0, FLOOR, return_terms=True)
        ratios[c] = np.array([d / m for d, m in zip(D, M)])
    allr = np.sort(np.unique(np.concatenate(list(ratios.values()))))
    tol, best = None, -1
    for lo, hi in zip(allr[:-1], allr[1:]):                    # candidates: the middles of the gaps between neighbouring ratios
        cand = 0.5 * (lo + hi)
        if min(abs(allr - cand) / cand) <= 1e-6:
            continue
        first = ratios[16] <= cand
        never = np.all([ratios[c] > cand for c in CHECKS], axis=0)
        between = ~first & ~never
        score = min(first.sum(), never.sum(), between.sum())
        if score > best:
            tol, best = cand, score
    return dict(flat=g["flat"], cam=cam, T=T, samples=samples, words_at=words_at, ratios=ratios, tol=float(tol))


def _ad48(case, **kw):
    return Ad(case["flat"], case["cam"], case["T"], W48, H27, SPP, DEPTH, SEED, n_chunks=SPP, min_chunks=16, check_chunks=16, **kw)


# ---- 1. an unreachable tolerance is the one-shot render ---------------------------------------------------------------------------
def _plain_words(a):
    """the words of rtw_render_accum_* over all chunks of a's render, on an accumulator of its own"""
    b = Ad(a.flat, a.cam, a.T, a.width, a.height, a.spp, a.depth, a.seed, a.n_chunks_arg)
    try:
        assert b.add(0, b.n_chunks) == 0
        return b.words().copy()
    finally:
        b.close()


@pytest.mark.usefixtures("numerics")
def test_unreachable_tolerance_equals_the_golden():
    import torch
    g = load_golden("cfg2_random_320x180_64spp_d16_f32")
    T = np.float32
    a = Ad(g["flat"], CamObj(g["cam"]), T, g["width"], g["height"], g["spp"], g["depth"], g["seed"], g["n_chunks"])
    try:
        d_img = torch.full((a.width * a.height * 3,), -1.0, dtype=torch.float32, device="cuda:0")
        a.run_ok(UNREACHABLE, d_out=d_img.data_ptr())
        assert (a.chunks() == a.n_chunks).all()
        ai = a.ainfo()
        assert ai["tiles_at_cap"] == ai["n_tiles"] == a.tiles_i * a.tiles_j and ai["tiles_converged"] == 0
        assert ai["rounds"] == 4                                  # 64 chunks, default checkpoints 16, 32, 48
        info = a.info()
        assert info["complete"] == 1 and info["samples_done"] == g["spp"] and info["chunks_done"] == a.n_chunks and a.ranges() == [(0, a.n_chunks)]
        torch.cuda.synchronize()
        assert _same(_image(d_img.cpu().numpy(), a.width, a.height), g["image"])
        assert _same(a.resolve(), g["image"])
        assert a.stats().segments == g["segments"] and a.stats().samples == g["width"] * g["height"] * g["spp"]
        assert np.array_equal(a.words()[..., :7], _plain_words(a)[..., :7])
    finally:
        a.close()


@pytest.mark.parametrize("name,width,height,spp,n_chunks,nch_cs", [("random_64x36_8spp_d50_f64", 64, 36, 8, 0, (8, 1)),
                                                                    ("random_64x36_8spp_d50_f64", 24, 13, 17, 6, (6, 3)),
                                                                    ("cfg2_random_320x180_64spp_d16_f32", 24, 13, 17, 6, (6, 3))])
def test_unreachable_tolerance_equals_the_single_render(name, width, height, spp, n_chunks, nch_cs):
    """Float64 and Float32, 1-sample chunks and 3-sample chunks with a short last chunk (17 = 5 x 3 + 2), checkpoints every 2 chunks"""
    g = load_golden(name)
    T = g["image"].dtype.type
    a = Ad(g["flat"], CamObj(g["cam"]), T, width, height, spp, 8, g["seed"], n_chunks, min_chunks=2, check_chunks=2)
    try:
        assert (a.n_chunks, a.chunk_spp) == nch_cs
        a.run_ok(UNREACHABLE, gamma=0)
        assert (a.chunks() == a.n_chunks).all() and a.ainfo()["rounds"] == a.n_chunks // 2
        assert a.ainfo()["samples"] == width * height * spp == a.stats().samples
        for gamma in (1, 0):
            assert _same(a.resolve(gamma), single(g["flat"], a.cam, T, width, height, spp, 8, g["seed"], n_chunks=n_chunks, gamma=gamma))
        assert np.array_equal(a.words()[..., :7], _plain_words(a)[..., :7])
    finally:
        a.close()


# ---- 2. word 7 is the oracle's half difference ------------------------------------------------------------------------------------
def test_words_are_the_oracle_sums_and_half_differences_one_sample_chunks(case48):
    a = _ad48(case48)
    try:
        a.run_ok(UNREACHABLE)
        w = a.words()
        assert np.array_equal(w, case48["words_at"][SPP])
        assert (w[..., 7].view(np.int64) != 0).any()
    finally:
        a.close()


def test_words_are_the_oracle_sums_and_half_differences_three_sample_chunks(oracle):
    g = load_golden("cfg2_random_320x180_64spp_d16_f32", numerics="reference")
    T, width, height, spp = np.float32, 24, 13, 17
    a = Ad(g["flat"], CamObj(g["cam"]), T, width, height, spp, 8, 3, n_chunks=6, min_chunks=2, check_chunks=2)
    try:
        assert (a.n_chunks, a.chunk_spp) == (6, 3)
        samples = all_samples(oracle, g["flat"], g["cam"], T, width, height, spp, 8, 3, 6)
        a.run_ok(UNREACHABLE)
        w = a.words()
        assert np.array_equal(w, oracle_words(samples, 3, [spp])[spp])
        assert (w[..., 7].view(np.int64) != 0).any()
    finally:
        a.close()


# ---- 3. the decisions are the rule's, on the oracle's samples --------------------------------------------------------------------
def test_tile_chunk_counts_are_the_rule_on_the_oracle_samples(case48):
    tol, ratios = case48["tol"], case48["ratios"]
    first = ratios[16] <= tol
    never = np.all([ratios[c] > tol for c in CHECKS], axis=0)
    allr = np.concatenate(list(ratios.values()))
    # the inputs: (a) a tile that stops at the first checkpoint, (b) one that never stops, (c) one in between, (d) no ratio near the tolerance
    assert first.any(), "(a)"
    assert never.any(), "(b)"
    assert (~first & ~never).any(), "(c)"
    assert (np.abs(allr - tol) > 1e-9 * tol).all(), "(d)"
    expect = rule_chunks(case48["words_at"], CHECKS, SPP, 1, W48, H27, tol, FLOOR)
    assert set(expect) >= {16, SPP} and len(set(expect)) >= 3
    a = _ad48(case48)
    try:
        a.run_ok(tol)
        assert np.array_equal(a.chunks(), expect)
        ai = a.ainfo()
        assert ai["tiles_converged"] == (expect < SPP).sum() and ai["tiles_at_cap"] == (expect == SPP).sum()
        assert (ai["min_chunks_held"], ai["max_chunks_held"]) == (16, SPP) and ai["tolerance"] == tol
        info = a.info()
        assert info["complete"] == 1 and info["chunks_done"] == 16 and info["samples_done"] == 16 and a.ranges() == [(0, 16)]
    finally:
        a.close()
    # the witness on the DEVICE's words after uniform passes: the prefix render of c chunks at an unreachable tolerance
    gpu_words = {}
    for c in CHECKS:
        b = Ad(case48["flat"], case48["cam"], case48["T"], W48, H27, c, DEPTH, SEED, n_chunks=c, min_chunks=16, check_chunks=16)
        try:
            gpu_words[c] = b.run_ok(UNREACHABLE).words().copy()
        finally:
            b.close()
        assert np.array_equal(gpu_words[c], case48["words_at"][c]), c
    assert np.array_equal(rule_chunks(gpu_words, CHECKS, SPP, 1, W48, H27, tol, FLOOR), expect)


# ---- 4. each tile is a prefix render ----------------------------------------------------------------------------------------------
def test_each_tile_is_the_prefix_render_of_its_chunk_count(case48):
    import torch
    a = _ad48(case48)
    try:
        d_img = torch.full((W48 * H27 * 3,), -1.0, dtype=torch.float32, device="cuda:0")
        a.run_ok(case48["tol"], d_out=d_img.data_ptr())
        torch.cuda.synchronize()
        img = a.resolve()
        assert _same(_image(d_img.cpu().numpy(), W48, H27), img)
        ct = a.chunks()
        assert len(set(ct)) >= 3
        for c in sorted(set(ct)):
            ref = single(case48["flat"], case48["cam"], case48["T"], W48, H27, min(SPP, int(c)), DEPTH, SEED, n_chunks=int(c))
            for t in range(ct.size):
                m = a.tile_mask(t)
                assert np.array_equal(img[m], ref[m]) == (ct[t] == c), (c, t)
    finally:
        a.close()


# ---- 5. scan mode, job size ---------------------------------------------------------------------------------------------------------
@pytest.mark.usefixtures("numerics")
def test_words_chunks_and_image_do_not_depend_on_scan_mode_or_job_size(case48):
    first = None
    for scan in SCANS:
        for jp in (1, 4, 16):
            a = _ad48(case48)
            try:
                a.run_ok(case48["tol"], flags=SCANS[scan], job_pixels=jp)
                got = (a.words().copy(), a.chunks(), a.resolve().copy(), a.ainfo()["samples"], a.stats().samples)
            finally:
                a.close()
            if first is None:
                first = got
                assert got[3] == got[4] and 16 in got[1]
            else:
                assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]) and _same(got[2], first[2]) and got[3:] == first[3:], (scan, jp)


def test_passes_of_one_run_may_mix_scan_modes_by_refinement(case48):
    """a refinement in another scan mode and job size continues the first run's words"""
    a, b = _ad48(case48), _ad48(case48)
    try:
        a.run_ok(1e9, flags=SCANS["cull"], job_pixels=16).run_ok(case48["tol"], flags=SCANS["valu"], job_pixels=1)
        b.run_ok(case48["tol"])
        assert np.array_equal(a.words(), b.words()) and np.array_equal(a.chunks(), b.chunks())
    finally:
        a.close()
        b.close()


# ---- 6. refinement ------------------------------------------------------------------------------------------------------------------
def test_refinement_equals_a_fresh_run(case48):
    tol = case48["tol"]
    a = _ad48(case48)
    try:
        a.run_ok(1e9)
        assert (a.chunks() == 16).all() and a.ainfo()["rounds"] == 1
        for t in (tol, tol, UNREACHABLE):
            before = a.chunks()
            a.run_ok(t)
            fresh = _ad48(case48)
            try:
                fresh.run_ok(t)
                assert np.array_equal(a.words(), fresh.words()) and np.array_equal(a.chunks(), fresh.chunks()) and _same(a.resolve(), fresh.resolve())
                assert a.ainfo()["samples"] == fresh.ainfo()["samples"] and a.info() == fresh.info()
            finally:
                fresh.close()
            assert (a.chunks() >= before).all()
        assert (a.chunks() == SPP).all()
        # a looser tolerance than the last is refused, nothing changes
        b = _ad48(case48)
        try:
            b.run_ok(tol)
            state = (b.words().copy(), b.chunks(), b.info(), b.ainfo())
            assert b.run(tol * 2) == -4 and b"looser" in b.L.rtw_last_error()
            assert b.run(tol, floor=FLOOR * 2) == -4 and b.run(tol, min_chunks=8) == -4 and b.run(tol, check_chunks=8) == -4
            assert b.run(tol, seed=SEED + 1) == -4 and b"another render" in b.L.rtw_last_error()
            assert np.array_equal(b.words(), state[0]) and np.array_equal(b.chunks(), state[1]) and (b.info(), b.ainfo()) == state[2:]
        finally:
            b.close()
    finally:
        a.close()


# ---- 7. bookkeeping, refusals on a device ------------------------------------------------------------------------------------------
def test_bookkeeping_and_refusals(case48):
    tol = case48["tol"]
    a = _ad48(case48)
    other = _ad48(case48)
    try:
        a.run_ok(tol)
        ct = a.chunks()
        expect = sum(a.npix(t) * min(SPP, int(ct[t])) for t in range(ct.size))
        assert a.ainfo()["samples"] == expect == a.stats().samples
        assert a.ainfo()["rounds"] == 1 + sum(1 for c in CHECKS if (ct > c).any())
        # plain passes, merges and blobs are refused on an adaptive accumulator; it stays as it is
        state = (a.words().copy(), a.info(), a.ainfo())
        assert a.add(60, 1) == -2 and b"adaptive" in a.L.rtw_last_error()
        assert other.add(0, 4) == 0
        assert a.L.rtw_accum_merge(a.acc, other.acc, None) == -2 and a.L.rtw_accum_merge(other.acc, a.acc, None) == -2
        size = C.c_uint64()
        assert a.L.rtw_accum_export(a.acc, None, 0, C.byref(size)) == -2
        assert np.array_equal(a.words(), state[0]) and (a.info(), a.ainfo()) == state[1:]
        # a uniform accumulator reads word 7 as 0, has no adaptive info, reports its prefix for every tile, and is refused as bound by plain passes
        assert not other.words()[..., 7].any() and other.words()[..., :6].any()
        st = other.C.AdaptiveInfo()
        assert other.L.rtw_accum_adaptive_info(other.acc, C.byref(st)) == -2
        assert (other.chunks() == 4).all()
        before = other.words().copy()
        assert other.run(tol) == -4 and b"plain passes" in other.L.rtw_last_error()
        assert np.array_equal(other.words(), before) and other.info()["chunks_done"] == 4
        # reset: a plain, empty accumulator again
        a.C.check(a.L.rtw_accum_reset(a.acc, None))
        assert a.info()["bound"] == 0 and not a.words().any() and a.L.rtw_accum_adaptive_info(a.acc, C.byref(st)) == -2
        assert a.add(0, SPP) == 0
        assert a.info()["complete"] == 1 and not a.words()[..., 7].any()
        assert _same(a.resolve(), single(case48["flat"], case48["cam"], case48["T"], W48, H27, SPP, DEPTH, SEED, n_chunks=SPP))
        # ... and an adaptive one after the next reset
        a.C.check(a.L.rtw_accum_reset(a.acc, None))
        a.run_ok(tol)
        assert np.array_equal(a.chunks(), ct) and np.array_equal(a.words(), state[0])
    finally:
        other.close()
        a.close()


# ---- 8. poison ----------------------------------------------------------------------------------------------------------------------
def test_a_poisoned_scene_finishes_and_stops_by_the_rule(rtw):
    """every albedo 1e12 (tests/test_gpu_accum.py test_poisoned_pixels_stay_poisoned): poisoned pixels add nothing to D and Y and
    resolve to NaN; the tiles stop where the rule, applied to the device's own prefix words, says.  The tolerance: q saturates at 64 per
    channel value while this scene's radiances reach 2^31, so D / Y is of the order 64 / 2^18; on the CPU oracle's samples of this
    frame the tiles' ratios at the first checkpoint spread over 0 .. 1e-3 with the median at 3e-4, and 2.5e-4 stops tiles at every one
    of the checkpoints 4, 8, 12 and leaves some running to 16"""
    T = np.float32
    flat = rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T)
    for k in ("ar", "ag", "ab"):
        flat[k] = np.full_like(flat[k], 1e12)
    cam = rtw.t_default_cam(elem_type=T)
    tol, checks = 2.5e-4, [4, 8, 12]
    a = Ad(flat, cam, T, 96, 54, 16, 4, 1, min_chunks=4, check_chunks=4)
    try:
        a.run_ok(tol)
        ct, w, img = a.chunks(), a.words(), a.resolve()
        poisoned = w[..., 6] > 0
        assert poisoned.any() and not poisoned.all()
        assert np.array_equal(np.isnan(img).any(axis=2), poisoned)
        words_at = {}
        for c in checks:
            b = Ad(flat, cam, T, 96, 54, c, 4, 1, n_chunks=c, min_chunks=4, check_chunks=4)
            try:
                words_at[c] = b.run_ok(UNREACHABLE).words().copy()
            finally:
                b.close()
        assert np.array_equal(ct, rule_chunks(words_at, checks, 16, 1, 96, 54, tol, FLOOR))
        some = [t for t in range(ct.size) if poisoned[a.tile_mask(t)].any()]
        assert some and len(set(ct)) > 1
        for c in sorted(set(ct)):
            ref = single(flat, cam, T, 96, 54, int(c), 4, 1, n_chunks=int(c))
            for t in np.nonzero(ct == c)[0]:
                m = a.tile_mask(t)
                assert _same(img[m], ref[m]), (c, t)
    finally:
        a.close()


# ---- 9. the Python layer ------------------------------------------------------------------------------------------------------------
def test_render_adaptive_and_adaptive_renderer(rtw, case48):
    T = np.float32
    scene = rtw.scene_random_spheres(elem_type=T)
    cam = rtw.t_cam1(elem_type=T)
    img, spp_map, info = rtw.render_adaptive(scene, cam, 64, 48, tolerance=0.05, depth=8, seed=3, min_chunks=16, check_chunks=16)
    assert img.shape == (36, 64, 3) and spp_map.shape == (36, 64) and spp_map.dtype == np.int32
    assert set(np.unique(spp_map)) <= {16, 32, 48} and int(spp_map.sum()) == info["samples"]
    for s in np.unique(spp_map):
        ref = rtw.render(scene, cam, 64, int(s), depth=8, seed=3, n_chunks=int(s))
        assert np.array_equal(img[spp_map == s], ref[spp_map == s])
    with rtw.AdaptiveRenderer(scene, cam, 64, 48, depth=8, seed=3, min_chunks=16, check_chunks=16, device=0) as ar:
        ar.run(1e9)
        assert (ar.tile_chunks() == 16).all() and ar.tile_chunks().shape == (5, 8)
        i2 = ar.run(0.05, group_cull=True)
        assert _same(ar.image(), img) and np.array_equal(ar.samples_per_pixel(), spp_map) and i2["samples"] == info["samples"]
        assert ar.info()["complete"] == 1 and ar.done
        from rtw_amd._capi import RtwError
        with pytest.raises(RtwError) as e:
            ar.run(0.1)
        assert e.value.code == -4
        with pytest.raises(RtwError) as e:
            ar.add()
        assert e.value.code == -2
