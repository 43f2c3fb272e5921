"""Resolve and merge on hand-made accumulator words (rtw_accum_kernels.hip accum_resolve_kernel, accum_merge_kernel, fx_to_double), reached with
no seam at all: rtw_accum_import takes a blob without a checksum, so tests/accum_words.py writes the header, the ranges and any words it
likes, and the imported accumulator is resolved, merged, read and exported like any other.  The words a render leaves are benign (small
positive sums, no ties, no carries between the halves); these are not: every shift count of the normalisation, exact ties and their
neighbours, the negation's carry, 2^127 - 1 and -2^127, carries in and out of every half of a merge.

The reference is exact: Python integers, one Fraction -> float step, single binary64 operations (accum_words.resolve / merge).  Frames
are 13 rows x 11 columns (143 pixels, 572 sixteen-byte pairs: two full blocks of the merge and a partial third) and 1 x 1.  Every
comparison is on the bits, NaNs by position.  Tolerance: NONE.

Out of scope, on purpose:
  * word 7 under merge -- plain accumulators hold 0 there and adaptive ones cannot be merged, exported or imported (its arithmetic in the
    stopping rule is in test_gpu_accum_kernels.py);
  * what a poison count that wraps at 2^64 MEANS -- no render can reach it; the one wrapping count below only pins that nothing is
    carried out of word 6 into word 7, as nothing is carried out of a channel;
  * the trace kernel itself -- its sums are pinned to the oracle in test_gpu_accum.py."""
import ctypes as C
import random

import numpy as np
import pytest

import accum_words as AW

pytestmark = pytest.mark.gpu

W, H = 11, 13
F = [np.float32, np.float64]
CAM = bytes((7 * k + 3) & 0xff for k in range(176))
# divisor -> the binding and ranges that hold it
BINDINGS = {
    1: dict(spp=1, chunk_spp=1, ranges=[(0, 1)]),
    3: dict(spp=3, chunk_spp=1, ranges=[(0, 3)]),
    1000: dict(spp=1000, chunk_spp=8, ranges=[(0, 125)]),
    2 ** 31 - 1: dict(spp=2 ** 31 - 1, chunk_spp=1, ranges=[(0, 2 ** 31 - 1)]),
    6: dict(spp=10, chunk_spp=4, ranges=[(0, 1), (2, 3)]),            # the last chunk is short: 4 + 2 samples
}


class Imported:
    """an accumulator made by rtw_accum_import (device 0), straight on the C ABI"""

    def __init__(self, blob):
        from rtw_amd import _capi
        self.C, self.L = _capi, _capi.lib()
        self.acc = C.c_void_p()
        blob = np.ascontiguousarray(blob)
        _capi.check(self.L.rtw_accum_import(0, blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(self.acc)))
        st = self.info()
        self.width, self.height = st["width"], st["height"]

    def resolve(self, gamma, T):
        out = np.empty(self.width * self.height * 3, T)
        fn = self.L.rtw_accum_resolve_host_f64 if T is np.float64 else self.L.rtw_accum_resolve_host_f32
        self.C.check(fn(self.acc, gamma, out.ctypes.data_as(C.c_void_p)))
        return AW.from_device_order(out, self.width, self.height, 3)

    def resolve_device(self, gamma, T):
        import torch
        d = torch.full((self.width * self.height * 3,), -1.0, dtype=torch.float64 if T is np.float64 else torch.float32, device="cuda:0")
        fn = self.L.rtw_accum_resolve_f64 if T is np.float64 else self.L.rtw_accum_resolve_f32
        self.C.check(fn(self.acc, gamma, C.c_void_p(d.data_ptr()), None))
        assert self.words() is not None                               # (read_pixels waits for the accumulator's event: the resolve is done)
        torch.cuda.synchronize()
        return AW.from_device_order(d.cpu().numpy(), self.width, self.height, 3)

    def words(self):
        out = np.empty(self.width * self.height * 8, np.uint64)
        self.C.check(self.L.rtw_accum_read_pixels(self.acc, out.ctypes.data_as(C.c_void_p)))
        return AW.from_device_order(out, self.width, self.height, 8)

    def info(self):
        st = self.C.AccumInfo()
        self.C.check(self.L.rtw_accum_info(self.acc, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def ranges(self):
        n = C.c_int32()
        self.C.check(self.L.rtw_accum_ranges(self.acc, 0, C.byref(n), None))
        buf = np.zeros(2 * n.value, np.int32)
        self.C.check(self.L.rtw_accum_ranges(self.acc, n.value, C.byref(n), buf.ctypes.data_as(C.POINTER(C.c_int32))))
        return [tuple(int(x) for x in r) for r in buf.reshape(-1, 2)]

    def export(self):
        size = C.c_uint64()
        self.C.check(self.L.rtw_accum_export(self.acc, None, 0, C.byref(size)))
        buf = np.empty(size.value, np.uint8)
        self.C.check(self.L.rtw_accum_export(self.acc, buf.ctypes.data_as(C.c_void_p), size.value, C.byref(size)))
        return buf

    def merge(self, other):
        return self.L.rtw_accum_merge(self.acc, other.acc, None)

    def close(self):
        if self.acc:
            self.C.check(self.L.rtw_accum_free(self.acc))
            self.acc = C.c_void_p()


def _blob(words, T, divisor, width=W, height=H, ranges=None):
    b = dict(BINDINGS[divisor])
    if ranges is not None:
        b["ranges"] = ranges
    return AW.blob(width, height, words, is_f64=T is np.float64, max_depth=16, seed=5, scene_hash=0xfeedfacecafebeef, cam=CAM, **b)


_frames = None


def class_frames():
    """the sums of accum_words.resolve_classes spread over as many 13 x 11 frames as they need, made once"""
    global _frames
    if _frames is None:
        vals = AW.resolve_classes()
        per = 3 * W * H
        _frames = [AW.words_of_sums(vals[k:k + per], W, H) for k in range(0, len(vals), per)]
    return _frames


def _check_resolves(words, T, divisor, width=W, height=H, device=True):
    a = Imported(_blob(words, T, divisor, width, height))
    try:
        assert a.info()["samples_done"] == divisor and a.info()["precision"] == (64 if T is np.float64 else 32)
        assert np.array_equal(a.words(), words)
        for gamma in (0, 1):
            ref = AW.resolve(words, divisor, gamma, T)
            assert AW.same_bits(a.resolve(gamma, T), ref), (divisor, gamma)
            if device:
                assert AW.same_bits(a.resolve_device(gamma, T), ref), (divisor, gamma)
        return ref
    finally:
        a.close()


@pytest.mark.parametrize("divisor", list(BINDINGS))
@pytest.mark.parametrize("T", F)
def test_resolve_of_every_class_of_sum(T, divisor):
    """0, +-1, 2^64; 2^b, 2^b +- 1 for every b (every shift count, the n = 63 / 64 / 65 seam between the words); exact ties with even and
    odd significands at every shift, and their neighbours one unit of 2^-64 away (a sticky bit in lo alone; rem = 0x3ff over a lo of all
    ones); all-ones significands that round into the next binade; 2^127 - 1, -2^127; hi = -1 with lo = 1 and lo = 0; random sums -- and
    the negative of each.  Negative sums under gamma are NaN, as sqrt gives; Float32 is the binary64 value rounded once more."""
    seen_nan = False
    for words in class_frames():
        ref = _check_resolves(words, T, divisor)                      # (returns the gamma = 1 reference)
        seen_nan = seen_nan or bool(np.isnan(ref).any())
    assert seen_nan and len(class_frames()) >= 5


@pytest.mark.parametrize("T", F)
def test_resolve_of_one_pixel_frames(T):
    t_even, t_odd = AW.tie(AW.TIE_SIGNIFICANDS[0], 54), AW.tie(AW.TIE_SIGNIFICANDS[2], 3)
    for rgb in ([t_even, t_even + 1, t_even - 1], [t_odd, -t_odd, t_odd + 1], [(1 << 127) - 1, -(1 << 127), 0], [1, -1, 1 << 64],
                [AW.signed128(1, AW.M64), AW.signed128(0, AW.M64), (1 << 63) - 1], [1 << 63, (1 << 63) + 1, (1 << 65) - 1]):
        for divisor in (1, 3, 6, 2 ** 31 - 1):
            _check_resolves(AW.words_of_sums(rgb, 1, 1), T, divisor, 1, 1)


@pytest.mark.parametrize("T", F)
def test_poisoned_pixels_resolve_to_nan_and_leave_their_neighbours_alone(T):
    rnd = random.Random(3)
    words = AW.words_of_sums([rnd.getrandbits(rnd.randint(1, 100)) for _ in range(3 * W * H)], W, H)
    poisoned = {(0, 0): 1, (12, 10): 2 ** 63, (5, 5): 2 ** 64 - 1, (6, 5): 1, (12, 0): 7}
    for (i, j), count in poisoned.items():
        words[i, j, 6] = count
    for divisor in (3, 6):
        a = Imported(_blob(words, T, divisor))
        try:
            for gamma in (0, 1):
                img = a.resolve(gamma, T)
                mask = np.isnan(img)
                for i in range(H):
                    for j in range(W):
                        assert mask[i, j].all() if (i, j) in poisoned else not mask[i, j].any(), (i, j)
                assert AW.same_bits(img, AW.resolve(words, divisor, gamma, T))
                assert AW.same_bits(a.resolve_device(gamma, T), img)
        finally:
            a.close()


# ---- merge --------------------------------------------------------------------------------------------------------------------------
def _merge_frames(seed):
    """two frames of random sums of random length (wraps modulo 2^128 included) with the named carries written over them;
    -> (a, b, {(i, j, channel): expected sum})"""
    rnd = random.Random(seed)

    def rand_sum():
        return rnd.getrandbits(rnd.randint(1, 128)) - (1 << 127 if rnd.random() < 0.5 else 0)

    a = AW.words_of_sums([rand_sum() for _ in range(3 * W * H)], W, H)
    b = AW.words_of_sums([rand_sum() for _ in range(3 * W * H)], W, H)
    for w in (a, b):
        for _ in range(6):
            w[rnd.randrange(H), rnd.randrange(W), 6] = rnd.getrandbits(20)
    M = AW.M64
    named = {
        (0, 0, 0): ((5 << 64) | (M - 6), (9 << 64) | 7, 15 << 64),                    # lo + lo wraps to exactly 0, with a carry
        (0, 0, 1): ((1 << 64) | M, (2 << 64) | M, (4 << 64) | (M - 1)),               # both lo 2^64 - 1
        (0, 0, 2): (-1, 1, 0),                                                        # hi:lo all ones + 1: the carry leaves the channel and is dropped
        (1, 0, 0): (123, 0, 123),                                                     # ... the next pixel's red is untouched
        (2, 0, 0): (-5, 9, 4), (2, 0, 1): (5, -9, -4), (2, 0, 2): (-(1 << 64), (1 << 64) + 1, 1),       # across zero, both ways
        (3, 0, 0): ((1 << 127) - 1, 1, -(1 << 127)), (3, 0, 1): (-(1 << 127), -1, (1 << 127) - 1),      # modulo 2^128
        (3, 0, 2): (-(1 << 127), -(1 << 127), 0),
        (12, 10, 0): (M, 1, 1 << 64), (12, 10, 2): (-(1 << 64), M, -1),                                 # the last pixel: the partial block
    }
    for (i, j, c), (sa, sb, _) in named.items():
        a[i, j, 2 * c], a[i, j, 2 * c + 1] = AW.split128(sa)
        b[i, j, 2 * c], b[i, j, 2 * c + 1] = AW.split128(sb)
    counts = {(0, 0): (0, 0, 0), (4, 0): (1, 2, 3), (5, 0): (0, 5, 5), (6, 0): (2 ** 63, 2 ** 63 - 1, 2 ** 64 - 1),
              (7, 0): (2 ** 64 - 1, 1, 0)}                                            # (the last: nothing is carried into word 7)
    for (i, j), (pa, pb, _) in counts.items():
        a[i, j, 6], b[i, j, 6] = pa, pb
    return a, b, {k: v[2] for k, v in named.items()}, {k: v[2] for k, v in counts.items()}


@pytest.mark.parametrize("T,ranges_a,ranges_b", [(np.float32, [(0, 1)], [(2, 3)]), (np.float64, [(1, 3)], [(0, 1)]), (np.float64, [(2, 3)], [(0, 1)])])
def test_merge_is_the_integer_sum(T, ranges_a, ranges_b):
    """10 samples in chunks of 4: the merged accumulator holds 4 + 2 = 6 samples in two ranges, or all 10 in one coalesced range"""
    wa, wb, named, counts = _merge_frames(11)
    a, b = Imported(_blob(wa, T, 6, ranges=ranges_a)), Imported(_blob(wb, T, 6, ranges=ranges_b))
    c = None
    try:
        assert a.merge(b) == 0
        got = a.words()
        ref = AW.merge(wa, wb)
        assert np.array_equal(got, ref)
        assert np.array_equal(b.words(), wb)                          # the source is only read
        for (i, j, ch), s in named.items():
            assert AW.signed128(got[i, j, 2 * ch], got[i, j, 2 * ch + 1]) == s, (i, j, ch)
        for (i, j), n in counts.items():
            assert int(got[i, j, 6]) == n, (i, j)
        assert not got[..., 7].any()
        merged = AW.coalesce(ranges_a + ranges_b)
        samples = AW.samples_held(merged, 10, 4)
        assert samples == (6 if len(merged) == 2 else 10)
        info = a.info()
        assert a.ranges() == merged and info["samples_done"] == samples and info["chunks_done"] == sum(e - s for s, e in merged)
        assert info["complete"] == (1 if samples == 10 else 0) and (info["spp"], info["chunk_spp"], info["n_chunks"]) == (10, 4, 3)
        images = {g: a.resolve(g, T) for g in (0, 1)}
        for g in (0, 1):
            assert AW.same_bits(images[g], AW.resolve(ref, samples, g, T)), g
        # overlapping chunks are refused and nothing moves
        assert a.merge(b) == -2 and np.array_equal(a.words(), ref)
        # export, free, import: the blob is the one the builder writes for the merged state; words and image come back
        blob = a.export()
        assert blob.tobytes() == _blob(ref, T, 6, ranges=merged).tobytes()
        a.close()
        c = Imported(blob)
        assert np.array_equal(c.words(), ref) and c.ranges() == merged and c.info() == info
        for g in (0, 1):
            assert AW.same_bits(c.resolve(g, T), images[g]), g
    finally:
        for x in (a, b, c):
            if x is not None:
                x.close()
