"""The plain matrix-pipe scan over its own sphere order (csrc/rtw_plain_layout.hpp: spatially sorted, evenly filled blocks of 32, ties by
the caller's index): the image is what it was.  Every render here is compared bit for bit, with equal `segments`, against the CPU oracle and
against the all-VALU scan (RTW_FLAG_SCAN_VALU, the caller's order) of the same scene.  Frames 64 x 36, 8 spp, depth 8 unless said
otherwise.  Tolerance: NONE."""
import numpy as np
import pytest

from test_plain_layout import blocks_of, build_tool

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 64, 36, 8, 8
#: spheres that go through the filter (everything but the ground sphere, which every lane tests by itself): one below a block edge, on it, above it
COUNTS = [31, 32, 33, 64, 65, 97]


def layer_scene(rtw, n_small, T, seed=7, extra=()):
    """a ground sphere of radius 1000 and `n_small` spheres of radius 0.2 scattered over a flat layer (x in -8 .. 8, z in -3 .. 3: the x
    axis is the widest), Lambertian / Metal / Dielectric in turn; `extra`: spheres appended behind them"""
    rng = np.random.default_rng(seed)
    s = rtw.HittableList()
    s.append(rtw.Sphere(np.array([0, -1000, 0], T), T(1000), rtw.Lambertian(np.array([0.5, 0.5, 0.5], T))))
    for k in range(n_small):
        c = np.array([rng.uniform(-8, 8), 0.2, rng.uniform(-3, 3)], T)
        alb = np.array(rng.uniform(0.1, 0.9, 3), T)
        mat = (rtw.Lambertian(alb), rtw.Metal(alb, T(rng.uniform(0, 0.5))), rtw.Dielectric(T(1.5)))[k % 3]
        s.append(rtw.Sphere(c, T(0.2), mat))
    for e in extra:
        s.append(e)
    return s


def camera(rtw, T):
    return rtw.default_camera((0, 6, 12), (0, 0, 0), (0, 1, 0), 40, 16 / 9, 0.1, 13.0, elem_type=T)


def check_scene(rtw, oracle, scene, T, depth=DEPTH, numerics="reference", cull=True):
    """matrix-pipe render == oracle == all-VALU render (== group cull), images and segments; returns the image"""
    cam = camera(rtw, T)
    img = rtw.render(scene, cam, W, SPP, depth=depth, seed=3, numerics=numerics)
    seg = rtw.last_stats()["segments"]
    assert rtw.last_stats()["samples"] == W * H * SPP
    ref, ost = oracle.render(rtw.flatten_scene(scene, T), cam, W, H, SPP, T=T, max_depth=depth, seed=3, numerics=numerics)
    bad = img != ref
    assert not bad.any(), f"{bad.sum()} of {bad.size} channels differ from the oracle; max abs diff {np.abs(img - ref).max()}"
    assert seg == ost["segments"]
    valu = rtw.render(scene, cam, W, SPP, depth=depth, seed=3, numerics=numerics, scan_valu=True)
    assert np.array_equal(img, valu) and rtw.last_stats()["segments"] == seg
    if cull:
        gc = rtw.render(scene, cam, W, SPP, depth=depth, seed=3, numerics=numerics, group_cull=True)
        assert np.array_equal(img, gc) and rtw.last_stats()["segments"] == seg
    return img


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n_small", COUNTS)
def test_block_edges(rtw, oracle, n_small, T):
    check_scene(rtw, oracle, layer_scene(rtw, n_small, T), T)


@pytest.mark.parametrize("numerics", ["reference", "contract", "reference_fma2"])
def test_numerics_modes(rtw, oracle, numerics):
    check_scene(rtw, oracle, layer_scene(rtw, 65, np.float32, seed=11), np.float32, numerics=numerics)


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_glass_sphere_at_depth_50(rtw, oracle, T):
    """paths inside the glass are not unit length (the reference does not renormalise): those rays take every sphere, the dead rows of
    the evenly filled blocks included, as a candidate"""
    glass = rtw.Sphere(np.array([0, 1, 0], T), T(1.0), rtw.Dielectric(T(1.5)))
    check_scene(rtw, oracle, layer_scene(rtw, 32, T, extra=[glass]), T, depth=50)


def _tie_scene(rtw, T, first, second, n_small=65, seed=21, ranks=None):
    """the layer scene with the spheres at caller indices `first` < `second` made one sphere (centre and radius) of two albedos.
    `ranks`: before that, the spheres of those two ranks along x are moved to the two indices (so the pair is the two spheres a kd
    split on x separates)."""
    s = layer_scene(rtw, n_small, T, seed=seed)
    if ranks is not None:
        order = sorted(range(1, len(s)), key=lambda i: (float(s[i].center[0]), i))
        for idx, rank in zip((first, second), ranks):
            j = order[rank]
            s[idx], s[j] = s[j], s[idx]
            order = sorted(range(1, len(s)), key=lambda i: (float(s[i].center[0]), i))
    c = np.array([float(s[first].center[0]), 0.6, float(s[first].center[2])], T)
    s[first] = rtw.Sphere(c.copy(), T(0.6), rtw.Lambertian(np.array([0.9, 0.1, 0.1], T)))
    s[second] = rtw.Sphere(c.copy(), T(0.6), rtw.Lambertian(np.array([0.1, 0.1, 0.9], T)))
    return s


def _blocks(scene, tmp_path):
    """block of every filter-class sphere of `scene` (index 0 is the ground sphere, tested in-lane), by caller index"""
    exe = build_tool(tmp_path)
    r = np.array([abs(float(sp.radius)) for sp in scene])
    assert r[0] >= 16 * np.sort(r)[len(r) // 2] and (r[1:] < 16 * np.sort(r)[len(r) // 2]).all()      # the upload's rule for "huge"
    nb, blk = blocks_of(exe, [[float(v) for v in sp.center] for sp in scene[1:]], tmp_path)
    return nb, np.concatenate([[-1], blk])


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", ["one_leaf", "two_blocks"])
def test_later_sphere_wins_a_tie(rtw, oracle, tmp_path, T, case):
    """two spheres with the same centre and radius, far apart in the caller's list: the later one is what the reference's scan returns,
    whichever rows of whichever blocks the two landed in"""
    if case == "one_leaf":
        first, second = 3, 60
        scene = _tie_scene(rtw, T, first, second)
        nb, blk = _blocks(scene, tmp_path)
        assert nb == 3 and blk[first] == blk[second]
    else:
        # 65 spheres in 3 leaves: the root's lower side is 1 leaf of 22 -- the spheres of ranks 21 and 22 along x are separated by it
        first, second = 5, 50
        scene = _tie_scene(rtw, T, first, second, ranks=(21, 22))
        nb, blk = _blocks(scene, tmp_path)
        assert nb == 3 and blk[first] != blk[second]
    img = check_scene(rtw, oracle, scene, T)
    # the pair is in the picture: with the two albedos exchanged the image is another one
    swapped = rtw.HittableList(scene)
    swapped[first] = rtw.Sphere(scene[first].center, scene[first].radius, scene[second].mat)
    swapped[second] = rtw.Sphere(scene[second].center, scene[second].radius, scene[first].mat)
    other = rtw.render(swapped, camera(rtw, T), W, SPP, depth=DEPTH, seed=3)
    assert not np.array_equal(img, other)


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_tie_where_the_later_sphere_has_the_smaller_device_index(rtw, oracle, T):
    """What the two cases above cannot see: the layout breaks equal coordinates by the caller's index, so of two identical spheres the
    earlier one always gets the smaller device index too, and a key built on the DEVICE index would pass them.  Here three identical
    ground spheres sit at caller indices 0, 20 and 50: the upload takes the first two as its huge spheres (tested in-lane, device
    indices behind the blocks: the largest), the third goes through the filter into a block (a small device index).  The reference's
    scan returns the third, the latest of the caller's list -- the ground has ITS albedo -- which only the original index in the key
    gets right: in-lane keys against a pass-2 key."""
    scene = layer_scene(rtw, 65, T, seed=5)
    for idx, alb in ((0, (0.8, 0.2, 0.2)), (20, (0.2, 0.8, 0.2)), (50, (0.2, 0.2, 0.8))):
        scene[idx] = rtw.Sphere(np.array([0, -1000, 0], T), T(1000), rtw.Lambertian(np.array(alb, T)))
    img = check_scene(rtw, oracle, scene, T)
    # the ground is blue: the image with the third sphere's albedo given to the first one instead is another one
    other = rtw.HittableList(scene)
    other[0], other[50] = scene[50], scene[0]
    assert not np.array_equal(img, rtw.render(other, camera(rtw, T), W, SPP, depth=DEPTH, seed=3))


_PROBE = """
import hashlib, sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import numpy as np, rtw_amd as R
from test_gpu_plain_layout import layer_scene, camera, W, SPP, DEPTH
for n in (32, 97):
    img = R.render(layer_scene(R, n, np.float32), camera(R, np.float32), W, SPP, depth=DEPTH, seed=3)
    print("sha", n, hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest())
"""


def test_scenes_of_more_than_one_block_take_their_own_order_and_the_aid_keeps_the_callers(rtw):
    """the environment switches are read once per process, so this test is about two fresh processes: the upload reports (RTW_DEBUG)
    which order the plain scan got -- 32 filter-class spheres: the caller's arrays; 97: its own order, 4 blocks; with
    RTW_PLAIN_ORDER=caller: the caller's order again (34 blocks' worth of rows: 4, the ground sphere in place) -- and the images agree"""
    import os
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    code = _PROBE.format(tests=tests, root=os.path.dirname(tests))
    out = {}
    for aid in ("", "caller"):
        env = dict(os.environ, RTW_ENABLE_TEST_AIDS="1", RTW_DEBUG="1", RTW_PLAIN_ORDER=aid)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        lay = [ln.split("layout: ")[1] for ln in r.stderr.splitlines() if "plain scan layout" in ln]
        out[aid] = (lay, [ln for ln in r.stdout.splitlines() if ln.startswith("sha")])
    assert out[""][0] == ["32 spheres through the filter, 2 blocks, the caller's order", "97 spheres through the filter, 4 blocks, its own order"]
    assert out["caller"][0] == ["32 spheres through the filter, 2 blocks, the caller's order", "97 spheres through the filter, 4 blocks, the caller's order"]
    assert out[""][1] == out["caller"][1] and len(out[""][1]) == 2


def test_batch_of_two_views(rtw, oracle):
    T = np.float32
    scene = layer_scene(rtw, 65, T)
    cams = [camera(rtw, T), rtw.default_camera((10, 3, 4), (0, 0, 0), (0, 1, 0), 35, 16 / 9, 0.0, 10.0, elem_type=T)]
    imgs = rtw.render_batch(scene, cams, W, SPP, depth=DEPTH, seed=[3, 4])
    flat = rtw.flatten_scene(scene, T)
    for v, cam in enumerate(cams):
        ref, _ = oracle.render(flat, cam, W, H, SPP, T=T, max_depth=DEPTH, seed=3 + v)
        assert np.array_equal(imgs[v], ref), v
        assert np.array_equal(imgs[v], rtw.render(scene, cam, W, SPP, depth=DEPTH, seed=3 + v, scan_valu=True)), v


def test_progressive_render_in_two_passes(rtw, oracle):
    T = np.float32
    scene = layer_scene(rtw, 65, T)
    cam = camera(rtw, T)
    with rtw.ProgressiveRenderer(scene, cam, W, SPP, depth=DEPTH, seed=3) as pr:
        pr.add(3)
        seg = pr.stats()["segments"]
        pr.add(SPP - 3)
        seg += pr.stats()["segments"]
        assert pr.done
        img = pr.image()
    ref, ost = oracle.render(rtw.flatten_scene(scene, T), cam, W, H, SPP, T=T, max_depth=DEPTH, seed=3)
    assert np.array_equal(img, ref)
    assert np.array_equal(img, rtw.render(scene, cam, W, SPP, depth=DEPTH, seed=3, scan_valu=True))
    assert seg == ost["segments"] == rtw.last_stats()["segments"]
