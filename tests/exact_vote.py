"""Exact model of the group cull's block vote on the matrix pipe (hit_world_mfma<.., CULLED>, the `block_sets` lambda of
raytracingweekend.jl_amd/csrc/rtw_scan_mfma.hpp), in rationals.  The checker's side of tests/test_gpu_cull_vote.py; a helper module.

The layout (which sphere sits at which device position, which positions are tested in-lane) is unit op 28's answer: block b is the positions
32 b .. 32 b + 31.  From it and the scene:
  * a block whose members are small spheres has the exact box min(c - |r|) .. max(c + |r|) over its members, in rationals.  The device holds that
    box rounded outwards to binary32 (rtw_scene.hip build_cull), so the exact box lies inside the device's;
  * a block that holds a BIG sphere (|r| > 4 x the lower median |r|) which is not in the in-lane list has the infinite box: every ray with a ray
    votes for it; a block whose members are all in the in-lane list, or that has none, is dead: nobody votes for it.

For a ray (o, d) as the kernel sees it -- its components rounded to binary32, for both precisions -- two sets of blocks:
  must   the blocks whose exact box the exact ray {o + t d, t >= 0} meets: the closed slab test in rationals, a zero component handled as a case.
         No tolerance.  (The design promises more: the box grown by the margin m.)  A vote that lacks one of these is a bug.
  may    the blocks whose exact box, grown per side and axis by the allowance A_k, overlaps the axis-aligned bounds of the exact ray clipped to the
         small class's exact box grown by A_k; a ray that misses that grown box gets the infinite boxes only.  A vote beyond it means the vote has
         stopped culling the way the design says it does.

The allowance, from the code and not from what the device answers.  block_sets clips the ray to the class box grown by m, takes the bounds
[pmin, pmax] of the segment's end points and looks up lo3 = pmin - 2 m, hi3 = pmax + 2 m in tables that pass a block when lo_b <= (upper edge of
the bin of hi3) and hi_b >= (lower edge of the bin of lo3), the edges moved outwards by RTW_CULL_EDGE_SLACK bins (rtw_cull_tables.hpp).  So a
block passes axis k only if  lo_b - [2 m + (1 + SLACK) w_k] <= pmax_k  and  hi_b + [...] >= pmin_k,  w_k the bin width (the class box's extent
/ 64).  On top of that: m = 1.001 x (the formula) in binary32 with 1-ulp hardware sqrt (2 x 1.001 + 1e-6 < 2.01, the rest of the 2.01 -- 0.4 %
of m, >= 1.5e-5 of the distances involved -- covers the rounding of tn, tf and the end points, a few 2^-24 of those distances, and the
reciprocals' ulp); the segment itself is the clip to a box grown by m <= A; the device's boxes are the exact ones moved outwards by at most
an ulp of binary32 twice (cluster box, block box), and its bin width comes from those boxes and a rounded reciprocal (<= one more SLACK bin):
    A_k = 2.01 m64 + (1 + 2 SLACK) w_k + 4 ulp32(L),
m64 = (2^-8 max(|d|^2, 1) + 2 sqrt(eps_p)) (|o - cs| + rs + 1), eps_p = max(|d|^2 - 1, 0) + 2.4e-7 |d|^2 -- block_sets' margin without its
1.001, in binary64 from the class's bounding sphere (cs, rs as build_cull and mfma_cull_of make them) --, L the largest magnitude among the
origin's and the class box's coordinates.  An axis on which the class has no extent has one bin for everything: A_k is infinite there.

A ray that does not use the filter (`ok` = 0: |o_k| > mf_o_max, |d|^2 > 1.0009, not finite) takes every live block, exactly; a lane without
a ray contributes nothing."""
from collections import namedtuple
from fractions import Fraction
import math

import numpy as np

from exact_filters import _fr

Layout = namedtuple("Layout", "idx inlane n_blocks")      # per device position: the caller's index or -1, in the in-lane list; blocks of 32
CULL_BINS = 64                                            # RTW_CULL_BINS
EDGE_SLACK = 1e-3                                         # RTW_CULL_EDGE_SLACK
DEAD, FINITE, BIG = 0, 1, 2


def layout_of(y):
    """op 28's rows (index, in-lane, positions, blocks) -> Layout"""
    npos, nb = int(y[0, 2]), int(y[0, 3])
    assert 0 < npos <= len(y) and npos % 32 == 0 and nb * 32 <= npos
    return Layout(y[:npos, 0].astype(np.int64), y[:npos, 1] != 0, nb)


def _clip(o, d, lo, hi):
    """the parameters t >= 0 at which o + t d lies in the closed box [lo, hi] (Fractions): (tn, tf), tf None for +inf; None: no such t"""
    tn, tf = Fraction(0), None
    for k in range(3):
        if d[k] == 0:
            if not (lo[k] <= o[k] <= hi[k]):
                return None
            continue
        t1, t2 = (lo[k] - o[k]) / d[k], (hi[k] - o[k]) / d[k]
        if t1 > t2:
            t1, t2 = t2, t1
        tn = max(tn, t1)
        tf = t2 if tf is None else min(tf, t2)
        if tn > tf:
            return None
    return tn, tf


class Model:
    def __init__(self, flat, layout, T):
        n = flat["n"]
        self.T = T
        self.c = np.stack([flat["cx"], flat["cy"], flat["cz"]], 1).astype(np.float64)
        self.r = np.asarray(flat["r"], np.float64)
        absr = np.abs(self.r)
        big = absr > 4.0 * np.sort(absr)[(n - 1) // 2]
        idx, inl = layout.idx, layout.inlane
        assert sorted(idx[idx >= 0].tolist()) == list(range(n)), "every sphere sits at exactly one device position"
        assert big[idx[inl]].all() and (idx[inl] >= 0).all(), "the in-lane list holds BIG spheres only"
        self.n_blocks = layout.n_blocks
        self.kind, self.lo, self.hi, self.members = [], [], [], []
        small = []
        for b in range(self.n_blocks):
            pos = [p for p in range(32 * b, 32 * b + 32) if idx[p] >= 0]
            mem = [int(idx[p]) for p in pos]
            self.members.append(mem)
            lo = hi = None
            if not mem:
                kind = DEAD
            elif big[mem].any():
                assert big[mem].all(), "a block is either of the small class or of the BIG class"
                kind = BIG if any(not inl[p] for p in pos) else DEAD
            else:
                kind = FINITE
                small += mem
                lo = [min(_fr(self.c[i, k]) - _fr(absr[i]) for i in mem) for k in range(3)]
                hi = [max(_fr(self.c[i, k]) + _fr(absr[i]) for i in mem) for k in range(3)]
            self.kind.append(kind); self.lo.append(lo); self.hi.append(hi)
        assert not (idx[32 * self.n_blocks:] >= 0).any() or all(inl[p] for p in range(32 * self.n_blocks, len(idx)) if idx[p] >= 0)
        self.finite = [b for b in range(self.n_blocks) if self.kind[b] == FINITE]
        self.big = frozenset(b for b in range(self.n_blocks) if self.kind[b] == BIG)
        self.live = frozenset(self.finite) | self.big
        self.glo = self.ghi = None
        if self.finite:
            self.glo = [min(self.lo[b][k] for b in self.finite) for k in range(3)]
            self.ghi = [max(self.hi[b][k] for b in self.finite) for k in range(3)]
            self.width = [(self.ghi[k] - self.glo[k]) / CULL_BINS for k in range(3)]
        # the class's bounding sphere as build_cull makes it (binary64 sums in device order) and mfma_cull_of hands it on (binary32)
        cs = np.zeros(3)
        for i in small:
            cs += self.c[i]
        if small:
            cs /= len(small)
        rs = max([math.sqrt(float(((self.c[i] - cs) ** 2).sum())) + absr[i] for i in small], default=0.0)
        c_rs = rs * (1.0 + 1e-5) + 1e-3 * float(np.abs(cs).sum()) * (1e-4 if T is np.float32 else 1e-12)
        self.cs = cs.astype(T).astype(np.float32).astype(np.float64)
        self.rs = float(np.float32(T(c_rs))) * 1.000001 + 1e-30
        self.small = small

    # ---- the allowance ----
    def margin64(self, o, d):
        """block_sets' margin without its factor 1.001, in binary64"""
        o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
        s2 = float((d * d).sum())
        eps_p = max(s2 - 1.0, 0.0) + 2.4e-7 * s2
        return (0.00390625 * max(s2, 1.0) + 2.0 * math.sqrt(eps_p)) * ((math.sqrt(float(((o - self.cs) ** 2).sum())) + self.rs) + 1.0)

    def allowance(self, o, d):
        """A_k per axis (Fractions; None: infinite)"""
        L = max(float(np.abs(np.asarray(o, np.float64)).max()), max(abs(float(v)) for v in self.glo + self.ghi))
        ulp = 2.0 ** (math.frexp(L)[1] - 24) if L > 0 else 0.0
        base = _fr(2.01 * self.margin64(o, d)) + 4 * _fr(ulp)
        return [None if self.width[k] == 0 else base + (1 + 2 * _fr(EDGE_SLACK)) * self.width[k] for k in range(3)]

    # ---- the two sets ----
    def must(self, o, d):
        fo, fd = [_fr(v) for v in o], [_fr(v) for v in d]
        return frozenset(b for b in self.finite if _clip(fo, fd, self.lo[b], self.hi[b]) is not None) | self.big

    def _segment(self, o, d):
        """(A, pmin, pmax) of the exact ray clipped to the class box grown by A, or (A, None, None)"""
        fo, fd = [_fr(v) for v in o], [_fr(v) for v in d]
        A = self.allowance(o, d)
        huge = Fraction(10) ** 40
        lo = [self.glo[k] - (A[k] if A[k] is not None else huge) for k in range(3)]
        hi = [self.ghi[k] + (A[k] if A[k] is not None else huge) for k in range(3)]
        seg = _clip(fo, fd, lo, hi)
        if seg is None:
            return A, None, None
        tn, tf = seg
        assert tf is not None, "a ray with a zero direction"
        a, e = [fo[k] + tn * fd[k] for k in range(3)], [fo[k] + tf * fd[k] for k in range(3)]
        return A, [min(a[k], e[k]) for k in range(3)], [max(a[k], e[k]) for k in range(3)]

    def may(self, o, d, excess_of=None):
        """the may set; with excess_of (a set of blocks): also the largest gap / A_k over those blocks and the axes (0: overlaps ungrown)"""
        if not self.finite:
            return self.big if excess_of is None else (self.big, 0.0)
        A, pmin, pmax = self._segment(o, d)
        out, worst = set(), 0.0
        for b in self.finite if pmin is not None else []:
            inside, frac = True, 0.0
            for k in range(3):
                gap = max(self.lo[b][k] - pmax[k], pmin[k] - self.hi[b][k], Fraction(0))
                if A[k] is not None:
                    inside = inside and gap <= A[k]
                    frac = max(frac, float(gap / A[k]))
            if inside:
                out.add(b)
                if excess_of is not None and b in excess_of:
                    worst = max(worst, frac)
        out = frozenset(out) | self.big
        return out if excess_of is None else (out, worst)

    def expected(self, o, d, ok):
        """(must, may) of a lane with a finite ray: a ray that does not use the filter takes every live block, exactly"""
        if not ok:
            return self.live, self.live
        return self.must(o, d), self.may(o, d)

    def word(self, blocks):
        w = 0
        for b in blocks:
            w |= 1 << b
        return w
