"""What the CPU oracle can say about the scenes of tests/big_scenes.py (tests/test_gpu_global_scene.py renders them on the GPU): the
special spheres are there and in the picture, the adaptive case is not vacuous, and the instance table covers every global-scene
instance."""
import numpy as np
import pytest

import big_scenes as BS

PREC = pytest.mark.parametrize("T", BS.PRECISIONS, ids=["f32", "f64"])


@PREC
def test_big_scene_has_its_special_spheres(T):
    for n in (BS.BIG[T],) + BS.BOUNDARY[T]:
        f = BS.scene(T, n)
        assert f["n"] == n and all(f[k].shape == (n,) and f[k].dtype == T for k in ("cx", "cy", "cz", "r", "ar", "ag", "ab", "param"))
        assert f["r"][0] == 1000 and (np.abs(f["r"][1:]) <= T(0.25)).all() and (np.abs(f["r"][1:]) >= T(0.05)).all()
        assert set(np.unique(f["kind"])) == {0, 1, 2}
        metal = f["kind"] == 1
        assert (f["param"][metal] >= 0).all() and (f["param"][metal] <= 0.5).all()
        assert f["kind"][BS.MIRROR] == 1 and f["param"][BS.MIRROR] == 0 and (f["param"][metal] > 0).any()
        # the hollow glass sphere: a negative radius inside a positive one, same centre
        o, i = BS.HOLLOW_OUTER, BS.HOLLOW_INNER
        assert f["kind"][o] == f["kind"][i] == 2 and f["r"][o] > 0 > f["r"][i] and -f["r"][i] < f["r"][o] and (f["r"] < 0).sum() == 1
        assert all(f[k][o] == f[k][i] for k in ("cx", "cy", "cz"))
        # the coincident pair: one centre, one radius, two albedos, far apart in the list
        a, b = BS.pair_indices(n)
        assert b - a > n // 2 and all(f[k][a] == f[k][b] for k in ("cx", "cy", "cz", "r", "kind"))
        assert any(f[k][a] != f[k][b] for k in ("ar", "ag", "ab"))


@PREC
def test_the_tie_and_the_hollow_sphere_are_in_the_picture(oracle, T):
    """the frame of the batch test's first view: with the pair's albedos exchanged, and with the hollow filled, the oracle's image is
    another one"""
    flat, cam = BS.scene(T), BS.cameras(T)[0]
    kw = dict(T=T, max_depth=8, seed=BS.VIEW_SEEDS[0], n_chunks=4, numerics="reference")
    ref, _ = oracle.render(flat, cam, 40, 22, 4, **kw)
    assert np.isfinite(ref).all()
    swapped, _ = oracle.render(BS.swapped_pair(flat), cam, 40, 22, 4, **kw)
    assert (ref != swapped).any()
    solid, _ = oracle.render(BS.solid_glass(flat), cam, 40, 22, 4, **kw)
    assert (ref != solid).any()


@PREC
def test_the_adaptive_case_is_not_vacuous(oracle, T):
    """at the tolerance picked from the oracle's samples at least 5 of the 24 tiles stop at the first checkpoint, at least 5 at a later
    one and at least 5 never, and no ratio is near the tolerance"""
    with oracle.numerics("reference"):
        case = BS.adaptive_case(oracle, T)
    tol, ratios = case["tol"], case["ratios"]
    first, later, never = BS.stop_groups(ratios, tol)
    assert first.size == 24 and first.sum() + later.sum() + never.sum() == 24
    assert first.sum() >= 5 and later.sum() >= 5 and never.sum() >= 5, (first.sum(), later.sum(), never.sum())
    allr = np.concatenate(list(ratios.values()))
    assert (np.abs(allr - tol) > 1e-6 * tol).all()


def test_the_table_covers_every_global_scene_instance():
    got = {c.expect for c in BS.CASES if c.expect.lds_scene == 0 and (c.expect.kernel == "features" or c.expect.batch or c.expect.accum)}
    assert got == BS.global_instances() and len(got) == 44
    for T in BS.PRECISIONS:                   # the boundary: lds_scene flips between the two sizes for the plain scans
        lo, hi = BS.BOUNDARY[T]
        for flags in (0, 4):
            rows = {c.n: c.expect.lds_scene for c in BS.CASES if c.T is T and c.flags == flags and c.entry == "render"}
            assert rows == {lo: 1, hi: 0}
