"""The paths a block can take through the block loop of hit_world_mfma (csrc/rtw_scan_mfma.hpp): neither ray half collects its sign bits,
only the first, only the second, both -- in a first, a middle and a partly filled last block, with lanes that have no ray and with a ray
that does not use the filter.  One wave of hand-made rays per case, unit ops 13 / 14 (closest hit) and their candidate sinks 19 / 20.

Scene: 70 spheres of radius 0.5 in three clusters 100 apart along x -- 32 + 32 + 6, in the caller's order, which is the block order of op
13; the kd split of the group cull (op 14) cuts the widest axis, x, at 64 and then at 32, so its blocks hold the same spheres.  A ray runs
along +z through one column of one cluster (it hits up to four spheres of that block) or passes 200 above everything.

Asserted: index and t_hit of every lane equal the oracle's closest hit bit for bit; the candidate sets cover the oracle's (the rule of
test_candidates_cover_the_oracle_and_the_band) and every pair inside the filter's guarantee band; and each case is what it claims to be --
by the oracle's discriminants alone the candidates lie in the intended (ray half, block) cells and in no other, and on the device the other
cells of a filter-using ray stay empty (those spheres are ~100 away: D ~ -1e4, against a band of the order of 1)."""
import numpy as np
import pytest

import exact_filters as X
from test_gpu_filters import centres, exact_classes, make_flat, oracle_sets, run_sink
from test_gpu_units import run_unit

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("numerics")]

N, BLOCKS = 70, [range(0, 32), range(32, 64), range(64, 70)]
MISS = ([0.0, 200.0, -50.0], [0.0, 0.0, 1.0])
TMIN = 1e-3


def scene(T):
    c = np.zeros((N, 3))
    for b, blk in enumerate(BLOCKS):
        for j, i in enumerate(blk):
            c[i] = [100.0 * (b - 1) + 0.01 * j, 3.0 * (j % 8), 3.0 * (j // 8)]
    return make_flat(c, np.full(N, 0.5), T)


def wave(flat, T, count=64, lo=None, hi=None, bad=None):
    """`count` rays, one per lane: lanes 0-31 aim at block `lo`, lanes 32-63 at block `hi` (None: they miss everything); lane `bad` gets
    the missing ray with |d|^2 = 1.0201 > 1.0009 -- not ok, every sphere is its candidate"""
    c, _ = centres(flat)
    o, d = [], []
    for lane in range(count):
        b = lo if lane < 32 else hi
        if b is None:
            oo, dd = MISS
        else:
            t = BLOCKS[b][lane % len(BLOCKS[b])]
            oo, dd = [c[t, 0] + 0.2, c[t, 1], -50.0], [0.0, 0.0, 1.0]
        if lane == bad:
            oo, dd = MISS[0], [0.0, 0.0, 1.01]
        o.append(oo); d.append(dd)
    return np.array(o, T).astype(np.float64), np.array(d, T).astype(np.float64)


#: name -> (arguments of wave(), the (ray half, block) cells that hold candidates)
CASES = {
    "a_none": (dict(), set()),
    "b_first_half_middle": (dict(lo=1), {(0, 1)}),
    "c_second_half_middle": (dict(hi=1), {(1, 1)}),
    "d_both_halves_middle": (dict(lo=1, hi=1), {(0, 1), (1, 1)}),
    "e_tail_first_half": (dict(lo=2), {(0, 2)}),
    "e_tail_second_half": (dict(hi=2), {(1, 2)}),
    "first_block_second_half": (dict(hi=0), {(1, 0)}),
    "f_first_half_40_lanes": (dict(lo=1, count=40), {(0, 1)}),
    "f_second_half_48_lanes": (dict(hi=1, count=48), {(1, 1)}),
    "f_first_half_20_lanes": (dict(lo=1, count=20), {(0, 1)}),
    "g_first_half_and_a_ray_off_the_filter": (dict(lo=1, bad=40), {(0, 1)}),
    "halves_in_different_blocks": (dict(lo=0, hi=2), {(0, 0), (1, 2)}),
}


def cells(sets, skip=None):
    """the (ray half, block) cells in which some ray has a member of `sets` [m, >= N]"""
    out = set()
    for lane in range(len(sets)):
        if lane == skip:
            continue
        for b, blk in enumerate(BLOCKS):
            if sets[lane, blk.start:blk.stop].any():
                out.add((lane // 32, b))
    return out


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_every_path_of_a_block(oracle, T, numerics):
    flat = scene(T)
    assert flat["n"] == N and -(-N // 32) == len(BLOCKS) == 3 and len(BLOCKS[2]) == 6          # a first, a middle and a partly filled last block
    cc, rr = centres(flat)
    assert (np.abs(rr) <= 4 * np.median(np.abs(rr))).all()                                      # no sphere leaves the filter for the in-lane classes
    s = X.mfma_scale(cc, rr)
    assert s is not None
    for name, (kw, want) in CASES.items():
        o, d = wave(flat, T, **kw)
        m, bad = len(o), kw.get("bad")
        tmax = np.full(m, np.inf)
        disc, dset, hset = oracle_sets(oracle, flat, o, d, TMIN, tmax, T)
        # the case is what it claims to be, by the oracle alone
        assert cells(dset, bad) == want and cells(hset, bad) == want, (name, cells(dset, bad))
        if bad is not None:
            assert not dset[bad].any()
        ref_idx, ref_t = oracle.hit_world_batch(flat, np.concatenate([o, d], 1).astype(T), T(TMIN), np.inf, T)
        assert {(l // 32, int(i) // 32) for l, i in enumerate(ref_idx) if i >= 0} == want, name
        x = np.concatenate([o, d, np.full((m, 1), float(T(TMIN))), np.full((m, 1), np.inf)], 1)
        band = X.mfma_band(o[:, None, :], cc[None], rr[None], s)
        _, _, s999 = exact_classes((name, T, "block_paths"), flat, o, d, band)
        for op in (13, 14):
            y = run_unit(op, x, 9, T, flat=flat)
            wrong = (y[:, 0].astype(np.int64) != ref_idx) | ((ref_idx >= 0) & (y[:, 1] != ref_t.astype(np.float64)))
            assert not wrong.any(), (name, op, numerics, np.flatnonzero(wrong)[:5], y[wrong][:3, :2], ref_idx[wrong][:3])
            ok, sc, cand, inl = run_sink(op, flat, o, d, float(T(TMIN)), tmax, T)
            assert not inl.any(), (name, op)
            want_ok = np.arange(m) != (-1 if bad is None else bad)
            assert np.array_equal(ok, want_ok), (name, op)
            lost = (hset if op == 14 else dset) & ~cand[:, :N]
            assert not lost.any(), (name, op, numerics, [(int(a), int(b)) for a, b in zip(*np.nonzero(lost))][:5])
            if op == 13:
                must = (s999 > 0) & ok[:, None]
                assert not (must & ~cand[:, :N]).any(), (name, op)
            # only the intended cells are ever collected for the rays that use the filter; the ray that does not takes every sphere
            assert cells(cand[:, :N], bad) == want, (name, op, cells(cand[:, :N], bad))
            if bad is not None:
                assert cand[bad, :N].all(), (name, op)
