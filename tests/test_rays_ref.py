"""Ray queries, CPU only: a census of the populations of tests/rays_ref.py on the oracle alone -- what keeps tests/test_gpu_rays.py
honest -- and the equivalence the ray kernel relies on: the oracle's bounded hit_world(tmin, tmax_i) is its unbounded scan followed by
"miss if tmax_i < t", index and record, for EVERY ray of every population."""
import numpy as np
import pytest

import rays_ref as RR

PRECISIONS = [np.float32, np.float64]


@pytest.fixture(scope="module", autouse=True)
def _reference_mode(oracle):
    with oracle.numerics("reference"):
        yield


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_every_population_of_the_485_sphere_scene_hits_and_misses(oracle, T):
    assert RR.scene("random", T)[0]["n"] in (485, 486)            # (scene_random_spheres(1): 485 spheres in Float32, one more in Float64)
    for k in RR.letters("random"):
        idx, rec = RR.reference("random", k, T)
        hits = float((idx >= 0).mean())
        print(f"{np.dtype(T).name} population {k}: {idx.size} rays, {hits:.3f} hits")
        assert hits >= 0.25 and 1.0 - hits >= 0.10, (k, hits)
        assert not rec[idx < 0].any() and not np.signbit(rec[idx < 0]).any()
        assert set(np.unique(rec[idx >= 0][:, 7])) <= {0.0, 1.0}


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_bounce_rays_reach_the_tmin_regime(oracle, T):
    idx, rec = RR.reference("random", "b", T)
    t = rec[idx >= 0][:, 0]
    assert (t < 1e-3).any() and (t >= T(RR.TMIN)).all(), np.sort(t)[:4]


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_limb_rays_fall_on_both_sides_at_every_k(oracle, T):
    idx, _ = RR.reference("random", "d", T)
    meta = RR.populations("random", T)["meta"]
    for k in RR.LIMB_K:
        at = idx[meta["d_k"] == k]
        assert (at >= 0).any() and (at < 0).any(), (k, at.tolist())


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_the_later_duplicate_wins_across_the_block_boundary(oracle, T):
    idx = np.concatenate([RR.reference("dup", k, T)[0] for k in RR.letters("dup")])
    assert RR.DUP_SECOND in idx and RR.DUP_PAIR[1] in idx
    assert RR.DUP_FIRST not in idx and RR.DUP_PAIR[0] not in idx
    t_idx = RR.reference("dup", "t", T)[0]
    assert t_idx[RR.DUP_FIRST] == RR.DUP_SECOND and t_idx[RR.DUP_PAIR[0]] == RR.DUP_PAIR[1]       # aimed at the earlier one's centre


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_every_tmax_choice_occurs_and_the_neighbours_flip(oracle, T):
    for name in RR.SCENES:
        pops = RR.populations(name, T)
        choice = pops["meta"]["e_choice"]
        assert set(choice.tolist()) == set(range(len(RR.TMAX_CHOICES))), name
        idx, _ = RR.reference(name, "e", T)
        a_idx, _ = RR.reference(name, "a", T)
        c = {w: choice == RR.TMAX_CHOICES.index(w) for w in RR.TMAX_CHOICES}
        assert (idx[c["t"]] >= 0).all() and (idx[c["above"]] >= 0).all() and (idx[c["below"]] < 0).all(), name     # the flip, on either side of t
        assert c["t"].any() and c["below"].any() and c["above"].any()
        assert (idx[c["tmin"]] < 0).all() and (idx[c["under_tmin"]] < 0).all() and np.array_equal(idx[c["inf"]], a_idx[c["inf"]])


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
@pytest.mark.parametrize("name", RR.SCENES)
def test_the_bounded_scan_is_the_unbounded_scan_with_tmax_applied_afterwards(oracle, name, T):
    flat, _ = RR.scene(name, T)
    rays, idx, rec, _ = RR.all_rays(name, T)
    open_rays = rays.copy()
    open_rays[:, 6] = np.inf
    u_idx, u_rec = RR.expected(flat, open_rays, T)
    b_idx, b_t = RR.unbounded(flat, rays, T)
    assert np.array_equal(b_idx, u_idx) and np.array_equal(RR.bits(b_t[u_idx >= 0]), RR.bits(u_rec[u_idx >= 0][:, 0]))     # the batched form is the same scan
    cut = (u_idx >= 0) & (rays[:, 6] < u_rec[:, 0])
    want_idx = np.where(cut, -1, u_idx).astype(np.int32)
    want_rec = np.where(cut[:, None], np.zeros_like(u_rec), u_rec)
    assert cut.any() and (~cut & (u_idx >= 0) & np.isfinite(rays[:, 6])).any()
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(RR.bits(rec), RR.bits(want_rec))
