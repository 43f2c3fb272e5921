"""The tile kernels of the adaptive render on hand-made words (rtw_accum_kernels.hip: tile_not_converged behind accum_tile_check_kernel and
accum_tile_check_batch_kernel; accum_tile_compact_kernel and the count / scan / scatter trio; accum_resolve_tiles_kernel), through
the unit ops 21-23 of rtw_unit_f64 -- adaptive accumulators can be neither exported nor imported, so these three have a seam.  The ops
launch the product's kernels through the launch helpers of the adaptive loop itself: the same grids.

Layouts (8-byte slots; "value": a binary64 number, integers as such; "raw": uint64 / int64; tiles of 8 x 8 pixels, n_tiles = ceil(H / 8) *
ceil(W / 8), tile t = (j / 8) * ceil(H / 8) + i / 8; words of pixel (i, j) at (j * H + i) * 8):
  op 21 tile check   count = n_views   in   value  width height c chunk_spp tolerance dark_floor 0 0
                                            per view: value C_t[n_tiles], raw words[W * H * 8]
                                       out  raw    per view flags[n_tiles] of the single check, launched view by view;
                                                   then flags[n_views * n_tiles] of ONE launch of the batched check
                                                   (1: C_t == c and NOT converged with n = c * chunk_spp;  0: every other tile)
  op 22 tile lists   count = n flags   in   raw    n slots, the low 32 bits of each are the flag
                                       out  raw    count, list[n] of the one-workgroup compaction; count, list[n] of count / scan /
                                                   scatter; list slots behind the count hold -1
  op 23 resolve      count = 1         in   value  width height spp chunk_spp gamma 0 0 0;  value C_t[n_tiles];  raw words[W * H * 8]
        (also rtw_unit_f32)            out  value  W * H * 3 results of type T, widened; the divisor of a pixel is min(spp, C_t * chunk_spp)

The witness of the stopping rule is rtw_amd.reference_decisions (pinned on the CPU in test_adaptive_abi.py); every hand-made frame of
accum_words.stopping_cases comes with the deviations from the rule that decide it the other way, and the test asserts that they do
before it looks at the kernel.  The lists are compared with np.flatnonzero, the resolve with accum_words.resolve and each tile's own
divisor.  Every comparison is exact.  Tolerance: NONE."""
import ctypes as C

import numpy as np
import pytest

import accum_words as AW

pytestmark = pytest.mark.gpu

W, H = 11, 13


def _call(op, count, x, n_out, out_dtype, T=np.float64):
    from rtw_amd import _capi
    L = _capi.lib()
    x = np.ascontiguousarray(x)
    y = np.full(n_out, -7, out_dtype)
    fn = L.rtw_unit_f64 if T is np.float64 else L.rtw_unit_f32
    _capi.check(fn(op, count, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), None, None))
    return y


def _values(*v):
    return np.array(v, np.float64).view(np.uint64)


def tile_check(views, width, height, c, cs, tol, floor):
    """``views``: [(C_t, words H x W x 8)] -> (flags of the single kernel, flags of the batch kernel), each n_views x n_tiles"""
    n_tiles = ((height + 7) // 8) * ((width + 7) // 8)
    parts = [_values(width, height, c, cs, tol, floor, 0, 0)]
    for chunks, words in views:
        assert len(chunks) == n_tiles and words.shape == (height, width, 8)
        parts += [_values(*chunks), AW.device_order(words, 8)]
    y = _call(21, len(views), np.concatenate(parts), 2 * len(views) * n_tiles, np.int64)
    return y[:len(views) * n_tiles].reshape(len(views), n_tiles), y[len(views) * n_tiles:].reshape(len(views), n_tiles)


def expected_flags(rtw, chunks, words, width, height, c, cs, tol, floor):
    conv = rtw.reference_decisions(words, width, height, c * cs, tol, floor)
    return ((np.asarray(chunks) == c) & ~conv).astype(np.int64)


# ---- the stopping rule ---------------------------------------------------------------------------------------------------------------
CASES = {cs["name"]: cs for cs in AW.stopping_cases()}


@pytest.mark.parametrize("name", list(CASES))
def test_stopping_rule_on_a_hand_made_frame(rtw, name):
    cs = CASES[name]
    args = (cs["words"], cs["width"], cs["height"], cs["c"] * cs["cs"], cs["tol"], cs["floor"])
    ref = rtw.reference_decisions(*args)
    for variant in cs["opposite"]:                                    # the case can tell the rule from each of these
        assert AW.decisions(*args, variant=variant)[cs["tile"]] != ref[cs["tile"]], variant
    want = expected_flags(rtw, cs["chunks"], cs["words"], cs["width"], cs["height"], cs["c"], cs["cs"], cs["tol"], cs["floor"])
    single, batch = tile_check([(cs["chunks"], cs["words"])], cs["width"], cs["height"], cs["c"], cs["cs"], cs["tol"], cs["floor"])
    assert list(single[0]) == list(want), (name, "single")
    assert list(batch[0]) == list(want), (name, "batch")


def test_other_chunk_counts_and_ragged_tiles_by_hand(rtw):
    """the expectations of three cases spelled out, not taken from the reference"""
    for name, want in (("ragged_at_equality", [0, 0, 0, 0]), ("ragged_above_equality", [1, 1, 1, 1]), ("other_chunk_counts", [1, 0, 0, 1]),
                       ("floor_times_n_first", [0, 0, 0, 0]), ("one_pixel_at_equality", [0]), ("one_pixel_above_equality", [1])):
        cs = CASES[name]
        single, batch = tile_check([(cs["chunks"], cs["words"])], cs["width"], cs["height"], cs["c"], cs["cs"], cs["tol"], cs["floor"])
        assert list(single[0]) == want and list(batch[0]) == want, name


def _median_tolerance(rtw, frames, width, height, n, floor):
    ratios = []
    for w in frames:
        _, D, _, M = rtw.reference_decisions(w, width, height, n, 1.0, floor, return_terms=True)
        ratios += [d / m for d, m in zip(D, M) if m > 0]
    return float(np.median(ratios))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_three_ragged_views_in_one_batch(rtw, seed):
    """three views with different words and different C_t: view v's flags of the one batched launch are its flags of its own launch,
    and both are the reference's -- twelve waves: three full workgroups"""
    frames = [AW.random_words(W, H, 10 * seed + v) for v in range(3)]
    c, cs, floor = 6, 3, 0.03
    tol = _median_tolerance(rtw, frames, W, H, c * cs, floor)
    chunks = [[6, 6, 6, 6], [6, 8, 6, 4], [6, 6, 12, 6]]
    want = np.stack([expected_flags(rtw, ch, w, W, H, c, cs, tol, floor) for ch, w in zip(chunks, frames)])
    if seed == 0:
        assert 0 < want.sum() < want.size
    single, batch = tile_check(list(zip(chunks, frames)), W, H, c, cs, tol, floor)
    assert np.array_equal(single, want) and np.array_equal(batch, want)


def test_five_one_pixel_views_in_one_batch(rtw):
    """five waves: a full workgroup and a partial one"""
    names = ["R_plus_G_first", "channels_rounded_before_the_sum"]
    frames = [CASES[n]["words"] for n in names]
    for h, poison in ((0, 0), ((1 << 57) + 32, 1), (1 << 40, 0)):
        w = AW.make_words(1, 1)
        AW.set_pixel(w, 0, 0, rgb=(AW.U(1 << 53), AW.U(1), AW.U(1)), h=h, poison=poison)
        frames.append(w)
    tol = 2.0 ** -20
    chunks = [[2], [2], [2], [2], [2]]
    want = np.stack([expected_flags(rtw, ch, w, 1, 1, 2, 1, tol, 0.0) for ch, w in zip(chunks, frames)])
    assert [int(x) for x in want[:, 0]] == [1, 1, 0, 0, 0]
    single, batch = tile_check(list(zip(chunks, frames)), 1, 1, 2, 1, tol, 0.0)
    assert np.array_equal(single, want) and np.array_equal(batch, want)
    # the same five with the third at another chunk count and the noisy ones swapped to the end
    order = [4, 3, 2, 1, 0]
    chunks2 = [[2], [2], [4], [2], [2]]
    frames2 = [frames[k] for k in order]
    want2 = np.stack([expected_flags(rtw, ch, w, 1, 1, 2, 1, tol, 0.0) for ch, w in zip(chunks2, frames2)])
    assert [int(x) for x in want2[:, 0]] == [0, 0, 0, 1, 1]
    single, batch = tile_check(list(zip(chunks2, frames2)), 1, 1, 2, 1, tol, 0.0)
    assert np.array_equal(single, want2) and np.array_equal(batch, want2)


# ---- the tile lists ------------------------------------------------------------------------------------------------------------------
def compact(flags):
    """int64 flags -> ((count, list) of the one-workgroup loop, (count, list) of count / scan / scatter)"""
    n = len(flags)
    y = _call(22, n, np.asarray(flags, np.int64).view(np.uint64), 2 * (n + 1), np.int64)
    return (int(y[0]), y[1:n + 1]), (int(y[n + 1]), y[n + 2:])


def _patterns(n):
    rng = np.random.default_rng(n)
    z = np.zeros(n, np.int64)
    pats = {"none": z.copy(), "all": np.ones(n, np.int64)}
    for name, k in (("first", 0), ("last", n - 1), ("index 1024", 1024), ("index 262144", 262144), ("index 1023", 1023)):
        if k < n:
            pats[name] = z.copy()
            pats[name][k] = 1
    pats["alternating"] = (np.arange(n) & 1).astype(np.int64)
    pats["half"] = (rng.random(n) < 0.5).astype(np.int64)
    pats["sparse"] = (rng.random(n) < 0.01).astype(np.int64)
    # any non-zero low half is a set flag: -1, 2, the sign bit alone; the high half of a slot is not part of the flag
    odd = rng.choice(np.array([0, 0, 1, -1, 2, 1 << 31, 0x7fffffff, 1 << 32, 5 << 40, (1 << 32) | 1], np.int64), n)
    pats["other values"] = odd
    return pats


@pytest.mark.parametrize("n", [1, 63, 64, 255, 256, 257, 1023, 1024, 1025, 2049, 3 * 1024 + 5, 262144 + 300])
def test_both_compactions_list_the_set_flags_in_order(n):
    """around the wave (64), the block of the trio (256) and the trip of the one-workgroup loop (1024); 262444 flags are 1026 blocks,
    so the scan kernel of the trio takes its second step of 1024 counts"""
    for name, flags in _patterns(n).items():
        want = np.flatnonzero(flags & 0xffffffff)
        for which, (count, lst) in zip(("loop", "trio"), compact(flags)):
            assert count == len(want), (n, name, which)
            assert np.array_equal(lst[:count], want), (n, name, which)
            assert (lst[count:] == -1).all(), (n, name, which)


# ---- the per-tile resolve -------------------------------------------------------------------------------------------------------------
_frames = None


def class_frames():
    global _frames
    if _frames is None:
        vals = AW.resolve_classes()
        per = 3 * W * H
        _frames = [AW.words_of_sums(vals[k:k + per], W, H) for k in range(0, len(vals), per)]
        _frames[0][3, 2, 6], _frames[0][12, 10, 6], _frames[1][8, 8, 6] = 1, 2 ** 63, 2 ** 64 - 1          # a few poisoned pixels
    return _frames


def resolve_tiles(words, chunks, width, height, spp, cs, gamma, T):
    x = np.concatenate([_values(width, height, spp, cs, gamma, 0, 0, 0), _values(*chunks), AW.device_order(words, 8)])
    y = _call(23, 1, x, width * height * 3, np.float64, T)
    back = y.astype(T)
    assert AW.same_bits(back.astype(np.float64), y)                   # (every slot holds a value of type T)
    return AW.from_device_order(back, width, height, 3)


@pytest.mark.parametrize("gamma", [0, 1])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_per_tile_resolve_of_every_class_of_sum(T, gamma):
    """1000 samples in chunks of 7: the four tiles hold 1, 3, 100 and 200 chunks -- 7, 21, 700 samples and, capped, 1000"""
    spp, cs, chunks = 1000, 7, [1, 3, 100, 200]
    div = AW.tile_divisors(chunks, W, H, spp, cs)
    assert sorted(set(div.reshape(-1))) == [7, 21, 700, 1000] and div[0, 0] == 7 and div[12, 0] == 21 and div[0, 10] == 700 and div[12, 10] == 1000
    for k, words in enumerate(class_frames()):
        assert AW.same_bits(resolve_tiles(words, chunks, W, H, spp, cs, gamma, T), AW.resolve(words, div, gamma, T)), k
    # one pixel, one tile, a divisor of one and the largest there is
    w = AW.words_of_sums([AW.tie(AW.TIE_SIGNIFICANDS[2], 60), -AW.tie(AW.TIE_SIGNIFICANDS[0], 1) - 1, (1 << 127) - 1], 1, 1)
    for spp1, cs1, c1 in ((1, 1, 1), (2 ** 31 - 1, 1, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (5, 2, 2)):
        div1 = AW.tile_divisors([c1], 1, 1, spp1, cs1)
        assert AW.same_bits(resolve_tiles(w, [c1], 1, 1, spp1, cs1, gamma, T), AW.resolve(w, div1, gamma, T)), (spp1, cs1, c1)
