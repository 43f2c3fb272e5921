"""The checker of the accumulator-word tests checked, CPU only: tests/accum_words.py (exact resolve / merge / stopping rule, the blob
builder, the hand-made frames) against the oracle's 64.64 sum, rational arithmetic, ``rtw_amd.reference_decisions`` and the library's
own blob validation; and the argument checks of the unit ops 21-23 (include/rtw_hip.h), which are decided before any HIP call.  The GPU
side is tests/test_gpu_accum_words.py (through import) and tests/test_gpu_accum_kernels.py (through the unit ops)."""
import ctypes as C
from fractions import Fraction
import os

import numpy as np
import pytest

import accum_words as AW


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="module")
def lib(rtw):
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def _fx_trunc(x):
    """one radiance as the kernel adds it: truncated towards zero at 2^-64"""
    q = int(abs(Fraction(float(x))) * 2 ** 64)
    return -q if x < 0 else q


def test_reference_resolve_agrees_with_the_oracles_sum(oracle):
    """the inputs of test_gpu_round2.test_exact_accumulation_unit: the oracle's __int128 accumulation rounds like Fraction -> float"""
    rng = np.random.default_rng(5)
    n = 4096
    x = rng.uniform(0, 4, (n, 8)) * rng.choice([1, 1, 1, 1e-3, 1e-9, 2.0 ** -40, -1, 1e6], (n, 8))
    x[0] = [0.1] * 8
    x[1] = [2.0 ** 31, 1, 1, 1, 1, 1, 1, 1]
    x[2] = [np.nan, 1, 1, 1, 1, 1, 1, 1]
    x[3] = [np.inf, 1, 1, 1, 1, 1, 1, 1]
    x[4] = [2.0 ** 31 - 1, 2.0 ** 31 - 1, 0.5, 2.0 ** -64, 2.0 ** -65, -2.0 ** -64, 0, 0]
    x[5] = [1.0, 2.0 ** -53, 2.0 ** -54, 0, 0, 0, 0, 0]
    x[6] = [-0.3, 0.3, 1e-20, -1e-20, 0, 0, 0, 0]
    sums, poison = [], []
    for i in range(n):
        ok = [v for v in x[i] if abs(v) < 2.0 ** 31]                 # (NaN, Inf and |x| >= 2^31 poison the pixel and add nothing)
        sums.append(sum(_fx_trunc(v) for v in ok))
        poison.append(8 - len(ok))
        s, bad = oracle.fx_sum(x[i])
        assert bad == poison[-1], i
        assert np.isnan(s) if bad else AW.sum_to_double(sums[-1]) == s, i
    # ... and through the frame-level helper: the first 143 sums in the red channel of a 13 x 11 frame, their poison counts in word 6
    w = AW.make_words(11, 13)
    for k in range(143):
        AW.set_pixel(w, k % 13, k // 13, rgb=(sums[k], 0, 0), poison=poison[k])
    img = AW.resolve(w, 1, 0, np.float64)
    for k in range(143):
        s, bad = oracle.fx_sum(x[k])
        px = img[k % 13, k // 13]
        assert np.isnan(px).all() if bad else (px[0] == s and px[1] == 0.0 and px[2] == 0.0), k


def test_the_tie_classes_are_ties():
    """by rational arithmetic, not by construction: tie(M, s) / 2^64 has two binary64 neighbours at the same distance, the reference
    picks the one with the even significand, and one unit of 2^-64 to either side decides it"""
    for M in AW.TIE_SIGNIFICANDS:
        for s in range(64):
            t = AW.tie(M, s)
            assert t < 1 << 127
            exact = Fraction(t, 1 << 64)
            below, above = Fraction(M << (11 + s), 1 << 64), Fraction((M + 1) << (11 + s), 1 << 64)
            lo, hi = float(below), float(above)
            assert Fraction(lo) == below and Fraction(hi) == above and np.nextafter(lo, np.inf) == hi        # adjacent binary64 numbers
            assert below < exact < above and exact - below == above - exact
            even = lo if M % 2 == 0 else hi
            assert AW.sum_to_double(t) == even and AW.sum_to_double(-t) == -even
            assert AW.sum_to_double(t + 1) == hi and AW.sum_to_double(t - 1) == lo
            assert AW.sum_to_double(-t - 1) == -hi and AW.sum_to_double(-t + 1) == -lo
    # the significand of all ones goes up into the next binade
    assert AW.sum_to_double(AW.tie((1 << 53) - 1, 0)) == 1.0 and AW.sum_to_double(((1 << 64) - 1) << 63) == 2.0 ** 63
    vals = AW.resolve_classes()
    assert len(vals) == len(AW.resolve_classes()) and vals == AW.resolve_classes()           # (deterministic)
    assert all(-(1 << 127) <= v < (1 << 127) for v in vals) and {0, 1, -1, 1 << 64, (1 << 127) - 1, -(1 << 127)} <= set(vals)
    assert all(AW.signed128(*AW.split128(v)) == v for v in vals)


def test_samples_held_and_merge_reference():
    assert AW.samples_held([(0, 1), (2, 3)], 10, 4) == 6 and AW.samples_held([(0, 3)], 10, 4) == 10
    assert AW.samples_held([(0, 2 ** 31 - 1)], 2 ** 31 - 1, 1) == 2 ** 31 - 1
    assert AW.coalesce([(2, 3), (0, 1)]) == [(0, 1), (2, 3)] and AW.coalesce([(1, 3), (0, 1)]) == [(0, 3)]
    a, b = AW.make_words(1, 2), AW.make_words(1, 2)
    AW.set_pixel(a, 0, 0, rgb=(AW.M64, -1, (1 << 127) - 1), poison=AW.M64)
    AW.set_pixel(b, 0, 0, rgb=(1, 1, 1), poison=1)
    m = AW.merge(a, b)
    assert [AW.signed128(m[0, 0, 2 * c], m[0, 0, 2 * c + 1]) for c in range(3)] == [1 << 64, 0, -(1 << 127)]
    assert not m[0, 0, 6:].any() and not m[1].any()


def test_variant_none_is_the_written_rule_and_every_case_discriminates(rtw):
    """``decisions(variant=None)`` is ``reference_decisions`` (pinned in test_adaptive_abi.py); on every hand-made frame each named
    deviation decides the case's tile the OTHER way, so a kernel with that deviation fails the GPU test of the case"""
    for seed in range(4):
        w = AW.random_words(11, 13, seed)
        for tol in (0.05, 0.2, 1.0):
            assert np.array_equal(AW.decisions(w, 11, 13, 6, tol, 0.03), rtw.reference_decisions(w, 11, 13, 6, tol, 0.03))
    seen = set()
    for cs in AW.stopping_cases():
        args = (cs["words"], cs["width"], cs["height"], cs["c"] * cs["cs"], cs["tol"], cs["floor"])
        ref = rtw.reference_decisions(*args)
        assert np.array_equal(AW.decisions(*args), ref), cs["name"]
        for variant in cs["opposite"]:
            assert AW.decisions(*args, variant=variant)[cs["tile"]] != ref[cs["tile"]], (cs["name"], variant)
            seen.add(variant)
    assert seen == set(AW.VARIANTS)
    by_name = {cs["name"]: cs for cs in AW.stopping_cases()}

    def ref_of(name):
        cs = by_name[name]
        return list(rtw.reference_decisions(cs["words"], cs["width"], cs["height"], cs["c"] * cs["cs"], cs["tol"], cs["floor"]))

    assert ref_of("D_in_lane_order") == [True] and ref_of("Y_in_lane_order") == [False] and ref_of("R_plus_G_first") == [False]
    assert ref_of("floor_times_n_first") == [True] * 4 and ref_of("equality_converges") == [True] and ref_of("below_equality") == [False]
    assert ref_of("ragged_at_equality") == [True] * 4 and ref_of("ragged_above_equality") == [False] * 4
    assert ref_of("one_pixel_at_equality") == [True] and ref_of("one_pixel_above_equality") == [False]
    assert ref_of("H_most_negative_plus_one") == [False] and ref_of("H_most_negative") == [True]
    assert ref_of("H_above_2p53_tie") == [True] and ref_of("H_above_2p53_up") == [False]


def _import(lib, b):
    h = C.c_void_p()
    rc = lib.rtw_accum_import(0, b.ctypes.data_as(C.c_void_p), b.size, C.byref(h))
    if h:
        lib.rtw_accum_free(h)
    return rc


def test_a_hand_built_bound_blob_passes_the_librarys_validation(lib):
    w = AW.words_of_sums(AW.resolve_classes()[:429], 11, 13)
    good = dict(is_f64=True, spp=10, chunk_spp=4, ranges=[(0, 1), (2, 3)], seed=9, scene_hash=0x1234, cam=bytes(range(176)))
    b = AW.blob(11, 13, w, **good)
    assert b.size == 248 + 16 + 143 * 64
    # the unbound form is byte for byte the one test_accum_abi.py writes
    assert AW.blob(2, 1).tobytes() == b"RTWACCUM" + np.array([1, 248], np.uint32).tobytes() + np.array([2, 1, 0, 0], np.int32).tobytes() + bytes(216 + 128)
    bad = [AW.blob(11, 13, w, **dict(good, n_chunks=4)), AW.blob(11, 13, w, **dict(good, spp=0, n_chunks=0)),
           AW.blob(11, 13, w, **dict(good, ranges=[(0, 2), (1, 3)])), AW.blob(11, 13, w, **dict(good, ranges=[(2, 4)])),
           AW.blob(11, 13, w, **dict(good, ranges=[(1, 1)])), AW.blob(11, 13, w, **dict(good, ranges=[], bound=1)), b[:-8]]
    for k, x in enumerate(bad):
        assert _import(lib, np.ascontiguousarray(x)) == -2, k
    if not _has_gpu():      # the well-formed blobs get as far as the device
        for x in (b, AW.blob(1, 1, None, spp=2 ** 31 - 1, ranges=[(0, 2 ** 31 - 1)]), AW.blob(11, 13, w, spp=1000, chunk_spp=8, ranges=[(0, 125)])):
            rc = _import(lib, x)
            assert rc > 0 or rc in (-21, -22), rc
            assert b"no HIP device" in lib.rtw_last_error()


def _unit(lib, op, count, x, y, f32=False):
    fn = lib.rtw_unit_f32 if f32 else lib.rtw_unit_f64
    return fn(op, count, x.ctypes.data_as(C.c_void_p) if x is not None else None, y.ctypes.data_as(C.c_void_p) if y is not None else None, None, None)


def test_the_accumulator_unit_ops_validate_before_any_hip_call(lib):
    """nulls -> -1; a bad size, a value the layout does not hold, or a call beyond the cap -> -2: the same answers with and without a device"""
    out = np.zeros(64, np.float64)
    head = np.zeros(8 + 1 + 8, np.float64)

    def check(**kw):
        h = head.copy()
        h[:6] = [kw.get("width", 1), kw.get("height", 1), kw.get("c", 2), kw.get("cs", 1), kw.get("tol", 0.5), kw.get("floor", 0.0)]
        h[6], h[8] = kw.get("pad", 0), kw.get("chunks", 2)
        return _unit(lib, 21, kw.get("count", 1), h, out)

    assert _unit(lib, 21, 1, None, out) == -1 and _unit(lib, 21, 1, head, None) == -1
    assert _unit(lib, 22, 1, None, out) == -1 and _unit(lib, 23, 1, None, out) == -1 and _unit(lib, 23, 1, head, None, f32=True) == -1
    assert _unit(lib, 24, 1, head, out) == -2 and b"unknown unit op" in lib.rtw_last_error()
    assert _unit(lib, 21, 1, head, out, f32=True) == -2 and _unit(lib, 22, 1, head, out, f32=True) == -2
    for bad in (dict(count=0), dict(count=-1), dict(width=0), dict(width=1.5), dict(height=-1), dict(width=16385), dict(width=2048, height=1024),
                dict(width=float("nan")), dict(c=-1), dict(c=2.5), dict(cs=0), dict(tol=0.0), dict(tol=float("inf")), dict(tol=float("nan")),
                dict(floor=-1.0), dict(floor=float("nan")), dict(pad=1), dict(chunks=-1), dict(chunks=0.5), dict(chunks=2.0 ** 31),
                dict(count=2 ** 21)):                             # (2^21 views of 1 + 8 slots: beyond the cap of 2^24 slots)
        assert check(**bad) == -2, bad
    flags = np.zeros(4, np.uint64)
    assert _unit(lib, 22, 0, flags, out) == -2 and _unit(lib, 22, -3, flags, out) == -2 and _unit(lib, 22, 2 ** 24 + 1, flags, out) == -2

    def resolve(f32=False, **kw):
        h = head.copy()
        h[:5] = [kw.get("width", 1), kw.get("height", 1), kw.get("spp", 4), kw.get("cs", 1), kw.get("gamma", 1)]
        h[5], h[8] = kw.get("pad", 0), kw.get("chunks", 2)
        return _unit(lib, 23, kw.get("count", 1), h, out, f32=f32)

    for bad in (dict(count=0), dict(count=2), dict(width=0), dict(height=2 ** 15), dict(spp=0), dict(cs=0), dict(cs=1.5), dict(gamma=2), dict(gamma=-1),
                dict(pad=1), dict(chunks=0), dict(chunks=1.25)):
        assert resolve(**bad) == -2 and resolve(f32=True, **bad) == -2, bad
    if not _has_gpu():      # the well-formed calls get as far as the device
        for rc in (check(), resolve(), resolve(f32=True), _unit(lib, 22, 4, flags, out)):
            assert rc > 0 or rc in (-21, -22), rc
            assert b"no HIP device" in lib.rtw_last_error()
