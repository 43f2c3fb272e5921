"""The hand-made waves of tests/list_cases.py, checked on the CPU: by the oracle alone every case is what it claims to be -- the oracle's
set {disc >= 0} of every ray equals the design, every other pair lies far outside both filters' bands (so the device can add no
candidate), the tie cases' winner is the last copy of the caller's list -- and by the restated rules (list_cases.model_*) the cases
reach what tests/test_gpu_list_caps.py pins: each boundary pair differs by ONE candidate and goes from 0 to exactly 1 early resolve, the
heavy case's pigeonhole bounds hold, and the tie arrangements cover every boundary.  The caps the cases rest on are read back from the
headers."""
import collections

import numpy as np
import pytest

import exact_filters as X
import list_cases as LC

F = [np.float32, np.float64]


def test_caps_are_the_sources():
    assert LC.source_caps() == (LC.PAIR_CAP, LC.CAP, LC.CAP2, LC.LIST_CAP) == (512, 160, 192, 16)
    # the unit kernel's list area is the one the cases assume: entries of two words, then the singles
    assert 2 * LC.CAP + LC.CAP2 == LC.PAIR_CAP


def test_the_rules_by_hand():
    """the restated rules on waves small enough to count on paper"""
    inc = np.zeros((64, 6 * 32), bool)
    for b in range(6):
        inc[np.arange(32), 32 * b + np.arange(32)] = True          # 32 entries per block, one bit each
    A, B, C, when = LC.model_mfma(inc)
    assert (A, B, C) == (1, 0, 0)                                   # 32, 64, 96, 128 | the fifth block finds 128 >= 97
    assert when[(0, 0)][0] == 0 and when[(0, 128)][0] == 1 and when[(0, 96)][:2] == (0, 0) and when[(0, 96)][2] == 1
    inc = np.zeros((64, 32), bool)
    inc[:, :16] = True                                             # 32 entries (H = 0) of 32 bits: iterations of 32 singles
    A, B, C, when = LC.model_mfma(inc)
    assert (A, B, C) == (0, 0, 6)                                   # 5 x 32 = 160 >= 129 in front of iterations 6, 11, 16, 21, 26, 31
    assert when[(32, 15)] == (0, 0, 0) and when[(0, 0)][1] == 6     # b = 31 first, b = 0 last
    inc = np.zeros((64, 64), bool)
    inc[7, :16] = True
    assert LC.model_valu(inc)[0] == 0
    inc[7, 40] = True
    D, when = LC.model_valu(inc)
    assert D == 1 and when[(7, 15)] == 0 and when[(7, 40)] == 1
    assert LC.model_cull_valu([[0] * k for k in (0, 1, 16, 17, 32, 33)]) == [0, 0, 0, 1, 1, 2]


@pytest.mark.parametrize("T", F, ids=["f32", "f64"])
@pytest.mark.parametrize("count", LC.COUNTS)
def test_cases_are_what_they_claim(oracle, count, T):
    from test_gpu_filters import centres, oracle_sets
    for case in LC.cases(count):
        flat = case.flat(T)
        o, d = case.rays(T)
        cc, rr = centres(flat)
        inc = case.incidence()
        # the design, by the oracle's deciding discriminant (in every numerics mode: the pairs are far from 0)
        for mode in ("reference", "contract", "reference_fma2"):
            with oracle.numerics(mode):
                disc, dset, hset = oracle_sets(oracle, flat, o, d, LC.TMIN, np.full(count, np.inf), T)
            assert np.array_equal(dset, inc) and np.array_equal(hset, inc), (case.name, mode)
        # every ray uses the filters, and no pair outside the design comes near a band (binary64 arithmetic on |D| >= 99 against bands < 1)
        s = X.mfma_scale(cc, rr)
        assert s is not None and X.f32_mf_ok(o, d, s).all() and X.f64_ok(o, d).all(), case.name
        band = np.maximum(X.mfma_band(o[:, None, :], cc[None], rr[None], s), X.f64_filter_band(o[:, None, :], cc[None], rr[None]))
        oc = o[:, None, :] - cc[None]
        D = rr[None] ** 2 - (oc[..., 0] ** 2 + oc[..., 1] ** 2)
        assert (band > 0).all() and (band[~inc] < 1).all(), (case.name, band.max())
        assert (D[~inc] < -64 * band[~inc] - 32).all(), case.name
        assert (D[inc] > 0.2).all(), case.name
        # the BIG class and the huge spheres are only where a case wants them
        if case.name != "B_inlane_filter":
            assert not LC.huge_of(case.r) and not LC.big_of(case.r), case.name
        # the claims, by the restated rules
        got, w13, w10 = LC.plain_counts(case)
        for k, v in case.exact.items():
            assert got[k] == v, (case.name, k, got)
        for k, v in case.at_least.items():
            if k != "E":
                assert got[k] >= v, (case.name, k, got)
        E = LC.model_cull_valu([np.flatnonzero(inc[l]) for l in range(count)])
        if "E" in case.at_least:
            assert min(E) >= case.at_least["E"]
        if case.tie:
            ref_idx, _ = oracle.hit_world_batch(flat, np.concatenate([o, d], 1).astype(T), T(LC.TMIN), np.inf, T)
            cp = case.copies(ref_idx)
            tied = [l for l in range(count) if len(cp[l]) >= 2]
            assert tied and all(ref_idx[l] == cp[l][-1] for l in tied), case.name


@pytest.mark.parametrize("count", LC.COUNTS)
def test_boundary_pairs_differ_by_one_candidate(count):
    pairs = collections.defaultdict(dict)
    for case in LC.cases(count):
        if case.pair:
            pairs[case.pair[0]][case.pair[1]] = case
    assert sorted(pairs) == ["A", "C", "DE"]
    for kind, two in pairs.items():
        lo, hi = two[0], two[1]
        diff = lo.incidence() != hi.incidence()
        assert diff.sum() == 1 and hi.incidence()[diff].all() and np.array_equal(lo.z, hi.z), kind
        g0, g1 = LC.plain_counts(lo)[0], LC.plain_counts(hi)[0]
        for k in ("D",) if kind == "DE" else (kind,):
            assert g0[k] == 0 and g1[k] == 1, (kind, g0, g1)
        e0 = LC.model_cull_valu([np.flatnonzero(lo.incidence()[l]) for l in range(count)])
        e1 = LC.model_cull_valu([np.flatnonzero(hi.incidence()[l]) for l in range(count)])
        if kind == "DE":
            lane = int(np.flatnonzero(diff.any(1))[0])
            assert not any(e0) and e1[lane] == 1 and sum(e1) == 1 and max(int(v) for v in lo.incidence().sum(1)) == 16


@pytest.mark.parametrize("count", LC.COUNTS)
def test_census_of_the_arrangements(oracle, count):
    """which arrangements of tied copies the cases reach under the plain ops (the cull ops' own order is censused on the device)"""
    T = np.float32
    c13, c10 = collections.Counter(), collections.Counter()
    got_B = None
    for case in LC.cases(count):
        got, w13, w10 = LC.plain_counts(case)
        print(count, case.name, "n =", case.n, got, "E =", sorted(set(LC.model_cull_valu([np.flatnonzero(r) for r in case.incidence()]))))
        if case.name == "heavy":
            inc = case.incidence()
            # candidates in both halves of at least 5 blocks, several per entry
            assert all(inc[l].reshape(-1, 2, 16).sum(2).min() >= 2 for l in range(count)) and case.n // 32 >= 5
        if case.name == "B_inlane_filter":
            huge, big = LC.huge_of(case.r), LC.big_of(case.r)
            assert len(huge) == 2 and len(big) - len(huge) >= 3 and len(big) <= 8 and set(huge) <= set(big)
            o, _ = case.rays(T)
            cc = case.centres(T)
            assert all((np.linalg.norm(o - cc[i], axis=1) < case.r[i] - 0.5).all() for i in big)          # every ray starts inside all of them
            # the group cull's in-lane list: the huge ones first, then the rest of the BIG class in the layout's order (= the caller's: build_cull)
            filt = [i for i in big if i not in huge]
            B = LC.model_mfma(LC.wave_rows(case.incidence()), exact=huge, inlane=filt)[1]
            got_B = B
            assert B == 1, B
        if case.tie:
            flat = case.flat(T)
            o, d = case.rays(T)
            ref_idx, _ = oracle.hit_world_batch(flat, np.concatenate([o, d], 1).astype(T), T(LC.TMIN), np.inf, T)
            cp = case.copies(ref_idx)
            t13, t10 = LC.classify_ties(case, cp, w13), LC.classify_ties(case, cp, w10)
            print("    ties, matrix pipe:", dict(collections.Counter(t13)), " VALU:", dict(collections.Counter(t10)))
            c13.update(t13); c10.update(t10)
    assert got_B == 1
    rel13 = {(r, o) for r, o, f in c13}
    assert {("round", "same"), ("C", "aligned"), ("C", "opposed"), ("A", "aligned")} <= rel13, rel13
    assert any(r in ("call", "C") and o == "opposed" and f == "first+" for r, o, f in c13), c13      # a farther, LATER sphere tested first: the Float64 kidx reset
    assert any(f == "after" for r, o, f in c13) and any(r == "A" for r, o, f in c13)
    assert {("A", "aligned", "first"), ("A", "aligned", "after"), ("A", "aligned", "mixed")} <= set(c10), c10
