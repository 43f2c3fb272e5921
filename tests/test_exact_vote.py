"""The exact model of the block vote (tests/exact_vote.py) and the rays of tests/vote_cases.py, checked on the CPU: the model on boxes
whose answer is known by hand, and -- on the recorded layouts of tests/golden/cull_layouts.npz -- that the rays make the assertions of
tests/test_gpu_cull_vote.py bite: enough (ray, block) pairs a vote MUST hold, enough it MUST NOT hold, in every block and every family."""
from fractions import Fraction

import numpy as np
import pytest

import exact_vote as V
import vote_cases as VC

F = [np.float32, np.float64]


def _two_boxes():
    """64 unit-free spheres of radius 1/4 on integer-ish centres: block 0 around x = 0 .. 3, block 1 around x = 20 .. 23 (a layout made by hand)"""
    T = np.float32
    cx = np.r_[np.arange(32) % 4, 20 + np.arange(32) % 4].astype(T)
    cy = np.r_[np.arange(32) // 4 % 4, np.arange(32) // 4 % 4].astype(T)
    cz = np.r_[np.arange(32) // 16, np.arange(32) // 16].astype(T)
    n = 64
    flat = dict(n=n, cx=cx, cy=cy, cz=cz, r=np.full(n, 0.25, T))
    return flat, V.Layout(np.arange(n), np.zeros(n, bool), 2), T


def test_model_on_two_boxes_by_hand():
    flat, lay, T = _two_boxes()
    M = V.Model(flat, lay, T)
    assert M.finite == [0, 1] and not M.big
    q = Fraction(1, 4)
    assert M.lo[0] == [-q, -q, -q] and M.hi[0] == [3 + q, 3 + q, 1 + q] and M.lo[1][0] == 20 - q and M.hi[1][0] == 23 + q
    assert M.glo == [-q, -q, -q] and M.ghi == [23 + q, 3 + q, 1 + q]
    # along x through both; started between them: the one ahead only; a zero component outside the slab: none
    assert M.must([-5, 1, 0.5], [1, 0, 0]) == {0, 1}
    assert M.must([10, 1, 0.5], [1, 0, 0]) == {1} and M.must([10, 1, 0.5], [-1, 0, 0]) == {0}
    assert M.must([10, 5, 0.5], [1, -0.0, 0]) == frozenset()
    # closed: on the face, through the corner, an ulp off it
    assert M.must([3.25, 1, 0.5], [1, 0, 0]) == {0, 1} and M.must([3.25, 1, 0.5], [0, 0, 1]) == {0}
    assert M.must([3.25 + 4, 3.25 - 4, 0], [-1, 1, 0]) == {0}
    assert M.must([float(np.nextafter(np.float32(7.25), np.float32(8))), -0.75, 0], [-1, 1, 0]) == frozenset()
    # the line crosses block 0 behind the origin only
    assert M.must([4, 1, 0.5], [1, 0, 0]) == {1}
    # may: the margin near the class is ~ 2^-8 x 15, the bins are 23.5 / 64 wide on x: a crossing ray along y between the blocks keeps clear
    o, d = [11.5, -3, 0.5], [0, 1, 0]
    A = M.allowance(o, d)
    assert 0.36 < float(A[0]) < 0.6 and float(A[1]) < 0.25
    assert M.may(o, d) == frozenset() and M.may([1, -3, 0.5], d) == {0}
    a1 = float(M.allowance([3.25 + float(A[0]), -3, 0.5], d)[0])          # (the margin grows with the distance to the class: A where the ray is)
    assert abs(a1 / float(A[0]) - 1) < 0.2
    assert M.may([3.25 + a1 * 0.99, -3, 0.5], d) == {0} and M.may([3.25 + a1 * 1.01, -3, 0.5], d) == frozenset()
    # a ray that misses the grown class box; one that does not use the filter; the vote word
    assert M.may([11.5, 9, 0.5], d) == frozenset()
    assert M.expected(o, d, False) == (M.live, M.live) and M.word(M.live) == 3
    # must is inside may
    for oo, dd in (([-5, 1, 0.5], [1, 0, 0]), ([3.25 + 4, 3.25 - 4, 0], [-1, 1, 0]), ([10, 1, 0.5], [0.6, 0.8, 0])):
        assert M.must(oo, dd) <= M.may(oo, dd)


def test_model_classes_of_blocks():
    """a BIG sphere outside the in-lane list makes its block's box infinite; with all of them in the list the block is dead"""
    flat, lay, T = _two_boxes()
    flat = dict(flat, n=66, cx=np.r_[flat["cx"], 0, 5].astype(T), cy=np.r_[flat["cy"], -100, 0].astype(T), cz=np.r_[flat["cz"], 0, 0].astype(T),
                r=np.r_[flat["r"], 99, 2].astype(T))
    idx = np.r_[np.arange(64), 64, 65, np.full(30, -1)]
    for inl, kind in (([True, False], V.BIG), ([True, True], V.DEAD)):
        M = V.Model(flat, V.Layout(idx, np.r_[np.zeros(64, bool), inl, np.zeros(30, bool)], 3), T)
        assert M.kind == [V.FINITE, V.FINITE, kind]
        assert M.must([11.5, 9, 0.5], [0, 1, 0]) == M.big == M.may([11.5, 9, 0.5], [0, 1, 0])
        assert M.live == {0, 1} | M.big


@pytest.mark.parametrize("T", F)
@pytest.mark.parametrize("name", VC.SCENES)
def test_rays_make_the_vote_assertions_bite(name, T):
    """the conditions on the INPUTS of the GPU test, from the model alone"""
    flat, M, fam, o, d, ok, must, may, fo, fd = VC.judged(name, T)
    assert 250 <= len(o) <= 700
    # the far-miss ray: uses the filter, votes for the infinite boxes only
    import exact_filters as X
    assert X.f32_mf_ok(fo[None], fd[None], X.mfma_scale(M.c, M.r))[0]
    assert M.must(VC.as_kernel(fo), fd) == M.big == M.may(VC.as_kernel(fo), fd)
    for j in range(len(o)):
        assert (must[j] is None) == (j >= len(o) - 2)
        if must[j] is not None:
            assert must[j] <= may[j] <= M.live, j
    nf = len(M.finite)
    if nf < 2:
        assert name == "one_block"
        return
    n_fam = len(VC.FAMILIES)
    in_must, out_may = np.zeros((n_fam, M.n_blocks), int), np.zeros((n_fam, M.n_blocks), int)
    pairs = either = 0
    for j in range(len(o)):
        if must[j] is None:
            continue
        for b in M.finite:
            pairs += 1
            in_must[fam[j], b] += b in must[j]
            out_may[fam[j], b] += b not in may[j]
            either += (b in may[j]) and (b not in must[j])
    stats = dict(scene=name, T=VC.tname(T), rays=len(o), blocks=nf, must=int(in_must.sum()), not_may=int(out_may.sum()), either=either, pairs=pairs)
    print(stats)
    assert in_must.sum() >= 100 and out_may.sum() >= 100, stats
    assert (in_must.sum(0)[M.finite] > 0).all() and (out_may.sum(0)[M.finite] > 0).all(), (stats, in_must.sum(0), out_may.sum(0))
    assert (in_must.sum(1) > 0).all() and (out_may.sum(1) > 0).all(), (stats, in_must.sum(1), out_may.sum(1))
    assert either <= pairs / 4, stats
    # rays of both kinds the range check knows
    assert (~ok[:-2]).sum() >= 8 and ok.sum() >= 0.9 * len(ok) - 16


@pytest.mark.parametrize("T", F)
def test_grazes_are_what_they_were_built_as(T):
    """the corner and edge grazes, by the model: on the lattice, whose corners both precisions hold, the ray through the corner and the one moved
    INTO the box by an ulp meet the block, the one moved off it by an ulp misses it exactly and stays inside the allowance; on the scene of two
    far-apart clumps the ray moved off by 0.4 of the class's size is beyond the allowance: the vote must not hold that block"""
    for name, outside in (("on_bin_edges", 0.4), ("two_clumps", 0.4)):
        flat, M, fam, o, d, ok, must, may, fo, fd = VC.judged(name, T)
        js = np.flatnonzero(fam == VC.FAMILIES.index("graze"))
        meta = VC.GRAZES[(name, T)]
        assert len(js) == len(meta) >= 64
        seen = {s: 0 for s in (0.0, -1.0, 1.0, outside)}
        for j, (b, shift) in zip(js, meta):
            assert ok[j]
            if name == "on_bin_edges" and shift in (0.0, -1.0):
                assert b in must[j], (j, b, shift)
                seen[shift] += 1
            if name == "on_bin_edges" and shift == 1.0:
                assert b not in must[j] and b in may[j], (j, b)
                seen[shift] += 1
            if name == "two_clumps" and shift == outside:
                assert b not in may[j], (j, b)
                seen[shift] += 1
        assert all(v >= 8 for s, v in seen.items() if (s == outside) == (name == "two_clumps")), seen
