"""The witness of the radiance queries (tests/trace_rays_ref.py) on the CPU oracle alone: its two forms agree on every ray the GPU tests
use, and the lists reach the regimes that matter.  No GPU, nothing of the library."""
import numpy as np
import pytest

import rays_ref as RR
import trace_rays_ref as TR

PRECISIONS = [np.float32, np.float64]


def _ab(oracle, name, T):
    for depth in TR.DEPTHS:
        a, b = TR.radiances_a(name, T, depth), TR.radiances_b(name, T, depth)
        assert a.shape == b.shape == (TR.rays_of(name, T)[0].shape[0], TR.MAX_SPP, 3)
        assert TR.same_words(a, b), f"{name} depth {depth}: {int((a.view(np.uint64) != b.view(np.uint64)).sum())} sample words differ between the two forms"
        for spp in TR.SPPS:
            assert TR.same_words(TR.resolve(a[:, :spp]), TR.resolve(b[:, :spp]))


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
@pytest.mark.parametrize("name", TR.SMALL_SCENES)
def test_the_two_forms_of_the_witness_agree(oracle, name, T):
    """(A) ray_color against (B) the loop restated from hit_world, scatter and skycolor: every sample of every ray of the scene's list, at
    every depth the GPU tests use, on the bits"""
    _ab(oracle, name, T)


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_the_two_forms_agree_in_every_numerics_mode(oracle, numerics, T):
    _ab(oracle, "random", T)


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_the_two_forms_agree_on_the_edge_list_and_the_big_scene(oracle, T):
    """the 1000 rays of the lane loop's edges (spp 3, depth 16; scaled directions and far origins among them) and the 64 rays of the scene
    the global-memory instances take (spp 2)"""
    for flat, rays, spp in ((RR.scene("random", T)[0], TR.edge_rays(T), 3), (RR.scene("big", T)[0], TR.big_rays(T), 2)):
        a = TR.sample_radiances(flat, rays, T, 16, spp)
        b = np.zeros_like(a)
        for i, ray in enumerate(rays):
            for s in range(spp):
                w = TR.walk(flat, ray[0:3], ray[3:6], oracle.rng_stream(TR.SEED, i, s), T, 16)
                if w["missed"]:
                    b[i, s] = w["rad"]
        assert TR.same_words(a, b)


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_census_of_the_lists(oracle, T):
    """what the lists reach, on the oracle alone: paths of 1, 2 and more than 16 / exactly 50 scans (cut off at every depth used), every
    material kind scattered from, a dielectric reflected and gone through, a Lambertian rejection loop of more than one trial, rays
    that start inside a sphere, rays whose samples differ"""
    kinds, lens = set(), set()
    through = reflected = long_reject = differing = cut16 = cut50 = inside = 0
    for name in TR.SMALL_SCENES:
        rays, where = TR.rays_of(name, T)
        assert 100 <= rays.shape[0] <= 260, (name, rays.shape)          # "about 200"; the two-sphere scene has four inside rays
        # the rays of population c start inside a sphere: |o - c_k| < |r_k| for some k, ray by ray
        flat = RR.scene(name, T)[0]
        cen = np.stack([np.asarray(flat[k], np.float64) for k in ("cx", "cy", "cz")], axis=1)
        rad_k = np.abs(np.asarray(flat["r"], np.float64))
        inside_rays = rays[where["c"]][:, 0:3].astype(np.float64)
        assert inside_rays.shape[0] >= 4
        for o in inside_rays:
            assert (np.linalg.norm(cen - o, axis=1) < rad_k).any(), (name, o.tolist())
        inside += inside_rays.shape[0]
        W = TR.walks(name, T)
        rad = TR.radiances_a(name, T, 16)
        for i, row in enumerate(W):
            for w in row:
                lens.add(w["n_scans"])
                cut16 += w["n_scans"] > 16 or (w["n_scans"] == 16 and not w["missed"])
                cut50 += not w["missed"]
                for k, dr, th in zip(w["kinds"], w["draws"], w["through"]):
                    kinds.add(k)
                    through += k == 2 and th
                    reflected += k == 2 and not th
                    long_reject += k == 0 and dr > 3
            differing += len({rad[i, s].tobytes() for s in range(TR.MAX_SPP)}) > 1
    assert kinds == {0, 1, 2}
    assert {1, 2, 3} <= lens and cut16 >= 1 and cut50 >= 1, (sorted(lens), cut16, cut50)
    assert through >= 10 and reflected >= 10 and long_reject >= 10 and differing >= 50 and inside >= 60, (through, reflected, long_reject, differing, inside)
    # the long-path list of the GPU tests: one ray inside the bubble that runs out of depth 50 among primary rays that miss at once
    ray, misses = TR.long_path_list(T)
    assert misses.shape[0] >= 100


def test_resolve_is_the_pixels_rule(oracle):
    """fx_sum per channel, one rounding, / spp; a sample that is NaN, infinite or >= 2^31 makes all three NaN"""
    rad = np.array([[[0.1, 0.2, 0.3], [0.7, 0.1, 0.0]], [[1.0, 2.0 ** 31, 0.5], [0.5, 0.5, 0.5]], [[np.nan, 0.0, 0.0], [1.0, 1.0, 1.0]],
                    [[2.0 ** 31 - 1.0, 0.25, 2.0 ** -40], [1.0, 0.5, 2.0 ** -41]]])
    out = TR.resolve(rad)
    assert np.isnan(out[1]).all() and np.isnan(out[2]).all() and not np.isnan(out[[0, 3]]).any()
    assert out[3, 0] == 2.0 ** 30 and out[3, 1] == 0.375 and out[3, 2] == 1.5 * 2.0 ** -41
    assert out[0, 0] == oracle.fx_sum([0.1, 0.7])[0] / 2.0
