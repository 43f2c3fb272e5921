"""Batched render on the GPU (include/rtw_hip.h rtw_render_batch_*): view v of a batch is bit-identical, in every channel, to the
single render of cams[v] with seeds[v] -- in every scan mode, numerics mode (conftest.numerics), precision and job size -- and the
batch's counters are the sums of the single renders'.  Tolerance: NONE."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN_CASES, CamObj, load_golden

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("numerics")]


def _frames(out, n, width, height):
    return out.reshape(n, width, height, 3).transpose(0, 2, 1, 3)


def single(flat, cam, T, width, height, spp, depth, seed, n_chunks=0, flags=0, job_pixels=0):
    from rtw_amd import _capi
    L = _capi.lib()
    S, keep = _capi.make_scene(flat, T)
    Cm = _capi.make_camera(cam, T)
    P = _capi.make_params(width=width, height=height, spp=spp, max_depth=depth, seed=seed, n_chunks=n_chunks, flags=flags,
                          job_pixels=job_pixels)
    out = np.empty(width * height * 3, T)
    fn = L.rtw_render_f64 if T is np.float64 else L.rtw_render_f32
    _capi.check(fn(C.byref(S), C.byref(Cm), C.byref(P), out.ctypes.data_as(C.c_void_p)))
    st = _capi.Stats()
    _capi.check(L.rtw_stats(C.byref(st)))
    return _frames(out, 1, width, height)[0], st


def batch(flat, cams, seeds, T, width, height, spp, depth, n_chunks=0, flags=0, job_pixels=0):
    from rtw_amd import _capi
    L = _capi.lib()
    S, keep = _capi.make_scene(flat, T)
    Cm = _capi.make_cameras(cams, T)
    sd = _capi.make_seeds(seeds, len(cams))
    P = _capi.make_params(width=width, height=height, spp=spp, max_depth=depth, seed=1, n_chunks=n_chunks, flags=flags,
                          job_pixels=job_pixels)
    out = np.empty(len(cams) * width * height * 3, T)
    fn = L.rtw_render_batch_f64 if T is np.float64 else L.rtw_render_batch_f32
    _capi.check(fn(C.byref(S), Cm, len(cams), sd, C.byref(P), out.ctypes.data_as(C.c_void_p)))
    st = _capi.Stats()
    _capi.check(L.rtw_stats(C.byref(st)))
    return _frames(out, len(cams), width, height), st


def _check_views(flat, cams, seeds, T, width, height, spp, depth, n_chunks=0, flags=0, job_pixels=0):
    """batch == the single renders, view by view and in the counters; returns the batch images"""
    imgs, st = batch(flat, cams, seeds, T, width, height, spp, depth, n_chunks, flags, job_pixels)
    seg = 0
    for v, (cam, seed) in enumerate(zip(cams, seeds)):
        ref, st1 = single(flat, cam, T, width, height, spp, depth, seed, n_chunks, flags)
        bad = imgs[v] != ref
        assert not bad.any(), f"view {v}: {bad.sum()} of {bad.size} channels differ; max abs diff {np.abs(imgs[v] - ref).max()}"
        seg += st1.segments
    assert st.segments == seg
    assert st.samples == len(cams) * width * height * spp
    assert st.sphere_tests == seg * int(flat["n"])
    return imgs


@pytest.mark.parametrize("scan", ["matrix", "valu"])
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_batch_of_three_views_matches_golden_and_single_renders(rtw, name, scan):
    """views: the golden camera, t_cam2 (aperture 2.0), the golden camera with another seed"""
    g = load_golden(name)
    T = g["image"].dtype.type
    cams = [CamObj(g["cam"]), rtw.t_cam2(elem_type=T), CamObj(g["cam"])]
    seeds = [g["seed"], g["seed"] + 11, g["seed"] + 1234567]
    imgs = _check_views(g["flat"], cams, seeds, T, g["width"], g["height"], g["spp"], g["depth"], g["n_chunks"], 4 if scan == "valu" else 0)
    assert np.array_equal(imgs[0], g["image"])
    assert not np.array_equal(imgs[2], imgs[0])          # (the seed is the view's own)


def test_group_cull_batch_of_four_cameras(rtw):
    g = load_golden("cfg2_random_320x180_64spp_d16_f32")
    T = np.float32
    cams = [CamObj(g["cam"]), rtw.t_cam1(elem_type=T), rtw.t_cam2(elem_type=T), rtw.t_default_cam(elem_type=T)]
    imgs = _check_views(g["flat"], cams, [g["seed"], 2, 3, 4], T, g["width"], g["height"], g["spp"], g["depth"], g["n_chunks"], flags=1)
    assert np.array_equal(imgs[0], g["image"])


@pytest.mark.parametrize("width,n_views", [(100, 3), (2, 1), (2, 5)])
def test_frames_not_a_multiple_of_eight(rtw, width, n_views):
    """jobs at the views' edges: 100 x 56 (tiles cut at the right and bottom), 2 x 1 (one pixel row of one tile per view)"""
    T = np.float32
    flat = rtw.flatten_scene(rtw.scene_random_spheres(elem_type=T), T)
    height = rtw.image_height(width)
    cams = [rtw.t_cam1(elem_type=T), rtw.t_cam2(elem_type=T), rtw.t_default_cam(elem_type=T)] * 2
    _check_views(flat, cams[:n_views], list(range(1, n_views + 1)), T, width, height, 8, 16)


def test_64_views_of_configs0(rtw):
    """BASELINE configs[0] (scene_2_spheres 96 x 54, 16 spp, depth 4) x 64 views: the batch the launch rules size like a large frame"""
    g = load_golden("cfg1_2spheres_96x54_16spp_d4_f32")
    T = np.float32
    base = [CamObj(g["cam"]), rtw.t_cam2(elem_type=T), rtw.t_default_cam(elem_type=T), rtw.t_cam1(elem_type=T)]
    cams = [base[v % 4] for v in range(64)]
    seeds = [g["seed"] + 7 * v for v in range(64)]
    imgs, st = batch(g["flat"], cams, seeds, T, g["width"], g["height"], g["spp"], g["depth"], g["n_chunks"])
    assert np.array_equal(imgs[0], g["image"])
    seg = 0
    for v in range(64):
        ref, st1 = single(g["flat"], cams[v], T, g["width"], g["height"], g["spp"], g["depth"], seeds[v], g["n_chunks"])
        assert np.array_equal(imgs[v], ref), v
        seg += st1.segments
    assert st.segments == seg and st.samples == 64 * 96 * 54 * 16


@pytest.mark.parametrize("job_pixels", [0, 1, 4, 8, 16])
def test_job_size_does_not_change_the_batch(rtw, job_pixels):
    g = load_golden("diel_plus_96x54_8spp_d16_f32")
    T = np.float32
    cams = [CamObj(g["cam"]), rtw.t_cam2(elem_type=T), rtw.t_cam1(elem_type=T)]
    seeds = [g["seed"], 5, 9]
    imgs, st = batch(g["flat"], cams, seeds, T, g["width"], g["height"], g["spp"], g["depth"], g["n_chunks"], job_pixels=job_pixels)
    assert np.array_equal(imgs[0], g["image"])
    for v in (1, 2):
        ref, _ = single(g["flat"], cams[v], T, g["width"], g["height"], g["spp"], g["depth"], seeds[v], g["n_chunks"])
        assert np.array_equal(imgs[v], ref), v


def test_device_batches_on_two_torch_streams(rtw):
    import torch
    T = np.float32
    scene = rtw.scene_2_spheres(elem_type=T)
    dr = rtw.DeviceRenderer(scene, rtw.t_default_cam(elem_type=T), device=0)
    cams_a = [rtw.t_default_cam(elem_type=T), rtw.t_cam2(elem_type=T)]
    cams_b = [rtw.t_cam1(elem_type=T), rtw.t_default_cam(elem_type=T), rtw.t_cam2(elem_type=T)]
    n = 96 * 54 * 3
    fa = torch.full((2 * n,), -1.0, dtype=torch.float32, device="cuda:0")
    fb = torch.full((3 * n,), -1.0, dtype=torch.float32, device="cuda:0")
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sa):
        dr.render_batch_into(fa.data_ptr(), cams_a, 96, 16, seeds=[3, 4], depth=4, n_elems=fa.numel(), stream=sa.cuda_stream)
    with torch.cuda.stream(sb):
        dr.render_batch_into(fb.data_ptr(), cams_b, 96, 16, seeds=[5, 6, 7], depth=4, n_elems=fb.numel(), stream=sb.cuda_stream)
    st = dr.stats()                                     # (the last batch issued from this thread: b)
    sa.synchronize(); sb.synchronize()
    with pytest.raises(ValueError):
        dr.render_batch_into(fa.data_ptr(), cams_b, 96, 16, n_elems=fa.numel(), stream=sa.cuda_stream)
    flat = rtw.flatten_scene(scene, T)
    ia, ib = _frames(fa.cpu().numpy(), 2, 96, 54), _frames(fb.cpu().numpy(), 3, 96, 54)
    seg = 0
    for imgs, cams, seeds in ((ia, cams_a, [3, 4]), (ib, cams_b, [5, 6, 7])):
        for v in range(len(cams)):
            ref, st1 = single(flat, cams[v], T, 96, 54, 16, 4, seeds[v])
            assert np.array_equal(imgs[v], ref)
            if cams is cams_b:
                seg += st1.segments
    assert st["segments"] == seg and st["samples"] == 3 * 96 * 54 * 16 and st["kernel_ms"] > 0
    dr.close()


def test_float64_batch_and_python_api(rtw):
    T = np.float64
    scene = rtw.scene_random_spheres(elem_type=T)
    cams = [rtw.t_cam1(elem_type=T), rtw.t_cam2(elem_type=T)]
    imgs = rtw.render_batch(scene, cams, 64, 8, seed=[1, 2])
    assert imgs.shape == (2, 36, 64, 3) and imgs.dtype == T
    st = rtw.last_stats()
    assert st["samples"] == 2 * 64 * 36 * 8
    for v in range(2):
        assert np.array_equal(imgs[v], rtw.render(scene, cams[v], 64, 8, seed=v + 1))
    same = rtw.render_batch(scene, cams, 64, 8, seed=1)                  # one int: every view's seed
    assert np.array_equal(same[1], rtw.render(scene, cams[1], 64, 8, seed=1))


def test_non_golden_view_against_the_live_oracle(rtw, oracle):
    T = np.float32
    scene = rtw.scene_random_spheres(elem_type=T)
    cams = [rtw.t_cam1(elem_type=T), rtw.t_cam2(elem_type=T)]
    imgs = rtw.render_batch(scene, cams, 64, 4, seed=[3, 9])
    ref, ost = oracle.render(rtw.flatten_scene(scene, T), cams[1], 64, 36, 4, T=T, max_depth=16, seed=9,
                             n_chunks=oracle.default_n_chunks(4), product_order=oracle.PRODUCT_FORWARD)
    assert np.array_equal(imgs[1], ref)
