"""The batched lens stages on the GPU (include/rtw_hip.h rtw_lens_batch_*, rtw_render_lens_batch_*) against the witness
tests/wide_aperture_ref.py (for max_radius <= 8: tests/defocus_ref.py through it).  Every comparison is on the BITS -- every view's image
and every region of every view's workspace; NaN values are compared as a set.  Tolerance: NONE.  The yardstick is the witness of view v,
never the single device call alone.  Frames (tests/lens_batch_ref.py SIZES): one pixel; partial tiles and partial blocks in both directions;
a one-pixel last small tile at both scales."""
import ctypes as C
import functools

import numpy as np
import pytest

import defocus_ref as FO
import lens_batch_ref as LB
import wide_aperture_ref as WA
from test_gpu_temporal_noise import _assert_same, _lib_layout, _ptr, _sfx

pytestmark = pytest.mark.gpu
PRECISIONS = [np.float32, np.float64]
GUARD = 64                          # bytes of sentinel in front of and behind the output and the workspace
SENTINEL = -7.0


@functools.lru_cache(maxsize=None)
def _views(size, T):
    W, H = size
    return LB.views(H, W, T)


@functools.lru_cache(maxsize=None)
def _witness(size, T, v, mr, gamma, frame=None):
    vs = _views(size, T)
    return LB.witness(vs[v], T, mr, gamma, None if frame is None else vs[frame])


def _bparams(max_radius, gamma, lens_radius=0.0, focus_dist=0.0):
    from rtw_amd import _capi
    return _capi.WideAperture(max_radius, 0, gamma, -1, (C.c_int32 * 2)(0, 0), lens_radius, focus_dist)


def _device(frames, lenses, T, mr, gamma, own_stream=False):
    """rtw_lens_batch_device_* -> per view (out [H, W, 3], the workspace's regions).  frames: the input frames (dicts image, features), as
    many as lenses or one; lenses: dicts cam, lens_radius, focus_dist.  The table is the restatement's (and the library's equals it); the
    output and the workspace start poisoned and sit between 64-byte sentinel guards that must survive; the inputs must stay"""
    import torch
    from rtw_amd import _capi
    L = _capi.lib()
    H, W = frames[0]["image"].shape[:2]
    n, nf = len(lenses), len(frames)
    eb = np.dtype(T).itemsize
    cams, lr, fd = [v["cam"] for v in lenses], [v["lens_radius"] for v in lenses], [v["focus_dist"] for v in lenses]
    table = LB.lens_table(cams, T, W, lr, fd)
    got = np.full((n, 32), SENTINEL, T)
    _capi.check(getattr(L, "rtw_lens_table_" + _sfx(T))(C.byref(_bparams(mr, gamma)), _capi.make_cameras(cams, T), n, W, H, (C.c_double * n)(*lr), (C.c_double * n)(*fd), _ptr(got)))
    assert FO.same_bits(got, table)
    host = [np.stack([_lib_layout(f[k]) for f in frames]) for k in ("image", "features")]
    dev = [torch.from_numpy(a).to("cuda:0") for a in host] + [torch.from_numpy(table).to("cuda:0")]
    dt = torch.float64 if T is np.float64 else torch.float32
    g = GUARD // eb
    one = L.rtw_wide_aperture_work_bytes(W, H, eb, mr)
    n_work = L.rtw_lens_batch_work_bytes(W, H, eb, mr, n)
    assert n_work == n * one and one == WA.work_elems(H, W, mr) * eb
    work = torch.full((n_work // eb + 2 * g,), SENTINEL, dtype=dt, device="cuda:0")
    out = torch.full((n * W * H * 3 + 2 * g,), SENTINEL, dtype=dt, device="cuda:0")
    stream = torch.cuda.Stream() if own_stream else None
    torch.cuda.synchronize()
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    _capi.check(getattr(L, "rtw_lens_batch_device_" + _sfx(T))(C.byref(_bparams(mr, gamma, float("nan"), -1.0)), n, nf, vp(dev[2]), W, H, vp(dev[0]), vp(dev[1]), vp(work, GUARD),
                                                               vp(out, GUARD), C.c_void_p(stream.cuda_stream) if own_stream else None))
    if own_stream:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    for d, h in zip(dev, host + [table]):
        assert FO.same_bits(d.cpu().numpy(), h)
    out_h, work_h = out.cpu().numpy(), work.cpu().numpy()
    for name, a in (("output", out_h), ("workspace", work_h)):
        assert (a[:g] == SENTINEL).all() and (a[-g:] == SENTINEL).all(), f"the guards of the {name} were written"
    outs = out_h[g:-g].reshape(n, W, H, 3).transpose(0, 2, 1, 3)
    works = work_h[g:-g].reshape(n, one // eb)
    return [(outs[v], WA.unpack_work(works[v], H, W, mr)) for v in range(n)]


def _assert_view(got, ref, what):
    assert list(got[1]) == list(ref[1]), what
    for name in ref[1]:
        _assert_same(got[1][name], ref[1][name], f"{what}: the workspace's {name}")
    _assert_same(got[0], ref[0], f"{what}: the image")


# ---- 1. the batch equals the witness ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mr", LB.RADII)
@pytest.mark.parametrize("size", LB.SIZES)
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_batch_equals_the_witness(T, size, mr):
    """three views, each with its own image, features, camera and lens (one with a focus override), gamma 0 and 1: every view's image and
    every region of every view's workspace is the witness's of that view; odd cases run on a stream of the caller's"""
    vs = _views(size, T)
    for gamma in (0, 1):
        got = _device(vs, vs, T, mr, gamma, own_stream=bool((gamma + mr // 16) % 2))
        for v in range(len(vs)):
            _assert_view(got[v], _witness(size, T, v, mr, gamma), f"max_radius {mr}, gamma {gamma}, view {v}")
    assert list(got[0][1]) == (["coc", "tile"] if mr <= 8 else list(WA.REGIONS))


# ---- 2. the bracket: one frame, four lenses ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(17, 33), (130, 5)])
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_bracket(T, size):
    """n_frames == 1: a closed aperture gives the input back on the bits (NaN where not valid); the camera's own focus and an override of
    it; two different K; each view equals the witness on that one frame"""
    vs = _views(size, T)
    frame = vs[1]                                              # (K = 6 px at the camera's own focus)
    own = dict(cam=frame["cam"], lens_radius=frame["lens_radius"], focus_dist=0.0)
    lenses = [dict(own, lens_radius=0.0), own, dict(own, focus_dist=6.0), dict(own, lens_radius=vs[2]["lens_radius"], focus_dist=2.5)]
    assert len({FO.host_constants(l["cam"], T, size[0], l["lens_radius"], l["focus_dist"], 32)[1] for l in lenses[1:]}) == 2
    for mr, gamma in ((32, 0), (16, 1), (8, 0)):
        got = _device([frame], lenses, T, mr, gamma, own_stream=mr == 16)
        for v, l in enumerate(lenses):
            ref = LB.witness(dict(frame, **l), T, mr, gamma)
            _assert_view(got[v], ref, f"max_radius {mr}, lens {v}")
        if gamma == 0:
            valid = ~np.isnan(got[0][1]["coc"][..., 1])
            assert valid.any() and not valid.all()
            assert FO.same_bits(got[0][0][valid], frame["image"][valid]) and np.isnan(got[0][0][~valid]).all()
        assert not FO.same_bits(got[1][0], got[2][0]) and not FO.same_bits(got[1][0], got[3][0])


# ---- 3. the view index beyond one grid row -----------------------------------------------------------------------------------------------------
def test_the_view_index_beyond_one_grid_row():
    """65 537 views of 1 x 1, Float32, max_radius 16: two more than one grid row of 65 535 holds, whatever the split of the view index over
    the grid's dimensions is.  The views cycle through four distinct (frame, lens) cases; every view's pixel and workspace is compared"""
    import torch
    from rtw_amd import _capi
    T, W, H, mr, n = np.float32, 1, 1, 16, 65537
    L = _capi.lib()
    cases = WA.handmade_cases(H, W, T, WA.SEEDS[T])
    kinds = [dict(image=cases[k]["image"], features=cases[k]["features"], cam=cases[k]["cam"], lens_radius=lr, focus_dist=fd)
             for k, lr, fd in ((5, cases[5]["params"]["lens_radius"], 6.0), (8, cases[8]["params"]["lens_radius"], 0.0), (10, cases[10]["params"]["lens_radius"], 0.0),
                               (8, cases[5]["params"]["lens_radius"], 2.0))]
    refs = [WA.wide_aperture(k["image"], k["features"], k["cam"], T, k["lens_radius"], k["focus_dist"], mr, 1) for k in kinds]
    assert len({r[0].tobytes() + r[1]["coc"].tobytes() for r in refs}) == 4            # four cases that differ
    kind_of = np.arange(n) % 4
    table4 = LB.lens_table([k["cam"] for k in kinds], T, W, [k["lens_radius"] for k in kinds], [k["focus_dist"] for k in kinds])
    table = np.ascontiguousarray(table4[kind_of])
    images = np.ascontiguousarray(np.stack([_lib_layout(k["image"]) for k in kinds])[kind_of])
    feats = np.ascontiguousarray(np.stack([_lib_layout(k["features"]) for k in kinds])[kind_of])
    dev = [torch.from_numpy(a).to("cuda:0") for a in (images, feats, table)]
    one = L.rtw_wide_aperture_work_bytes(W, H, 4, mr) // 4
    g = GUARD // 4
    work = torch.full((n * one + 2 * g,), SENTINEL, dtype=torch.float32, device="cuda:0")
    out = torch.full((n * 3 + 2 * g,), SENTINEL, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    _capi.check(L.rtw_lens_batch_device_f32(C.byref(_bparams(mr, 1)), n, n, vp(dev[2]), W, H, vp(dev[0]), vp(dev[1]), vp(work, GUARD), vp(out, GUARD), None))
    torch.cuda.synchronize()
    out_h, work_h = out.cpu().numpy(), work.cpu().numpy()
    for a in (out_h, work_h):
        assert (a[:g] == SENTINEL).all() and (a[-g:] == SENTINEL).all()
    outs, works = out_h[g:-g].reshape(n, 3), work_h[g:-g].reshape(n, one)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for k in range(4):
        sel = kind_of == k
        first = int(np.flatnonzero(sel)[0])
        # every view of this kind equals the first one on the bits (the padding between the regions keeps its sentinel in all of them) ...
        assert (bits(outs[sel]) == bits(outs[first])).all() and (bits(works[sel]) == bits(works[first])).all(), k
        # ... and the first one, like the last view of the batch when it is of this kind, equals the witness
        for v in {first, int(np.flatnonzero(sel)[-1])}:
            _assert_view((outs[v].reshape(1, 1, 3), WA.unpack_work(works[v], H, W, mr)), refs[k], f"view {v} (kind {k})")
    assert kind_of[n - 1] == 0 and n - 1 == 65536


# ---- 4. host form equals device form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_host_forms_equal_the_device_form(rtw, T):
    """wide_aperture_batch and focus_bracket (the Python layer over rtw_lens_batch_*) against the device results -- and thereby the witness"""
    size = (33, 17)
    vs = _views(size, T)
    cams = [LB.as_camera(v["cam"], T) for v in vs]
    lr, fd = [v["lens_radius"] for v in vs], [v["focus_dist"] for v in vs]
    for mr, gamma in ((32, 1), (8, 0)):
        dev = _device(vs, vs, T, mr, gamma)
        got = rtw.wide_aperture_batch(np.stack([v["image"] for v in vs]), np.stack([v["features"] for v in vs]), cams, lens_radii=lr, focus_dists=fd, max_radius=mr,
                                      gamma=bool(gamma), device=0)
        assert got.shape == (3, size[1], size[0], 3) and got.dtype == T
        for v in range(3):
            _assert_same(got[v], dev[v][0], f"wide_aperture_batch, max_radius {mr}, view {v}")
            _assert_same(got[v], _witness(size, T, v, mr, gamma)[0], f"wide_aperture_batch against the witness, view {v}")
        focus = [0.0, 6.0, 2.5]
        lenses = [dict(cam=vs[1]["cam"], lens_radius=vs[1]["lens_radius"], focus_dist=f) for f in focus]
        dev = _device([vs[1]], lenses, T, mr, gamma)
        got = rtw.focus_bracket(vs[1]["image"], vs[1]["features"], cams[1], focus_dists=focus, lens_radius=vs[1]["lens_radius"], max_radius=mr, gamma=bool(gamma), device=0)
        assert got.shape == (3, size[1], size[0], 3)
        for v in range(3):
            _assert_same(got[v], dev[v][0], f"focus_bracket, max_radius {mr}, lens {v}")


# ---- 5. the one-call form ------------------------------------------------------------------------------------------------------------------------
DENOISE = dict(levels=2, sigma_color=0.7)


def _cameras(rtw, T):
    """the two spheres from three sides through apertures of about 1: K = 0.5 * 96 / |horizontal| is about 13 px at 96 x 54"""
    kw = dict(lookat=(0, 0, -1), vup=(0, 1, 0), vfov=30, aspect_ratio=16 / 9, elem_type=T)
    return [rtw.default_camera(lookfrom=(3, 1, 2), aperture=1.0, focus_dist=3.7, **kw), rtw.default_camera(lookfrom=(-2.5, 1.5, 2.5), aperture=0.9, focus_dist=4.0, **kw),
            rtw.default_camera(lookfrom=(2, 0.75, 3), aperture=1.1, focus_dist=3.5, **kw)]


@pytest.mark.parametrize("gamma", [False, True], ids=["linear", "gamma"])
@pytest.mark.parametrize("denoise", [None, DENOISE], ids=["plain", "filtered"])
@pytest.mark.parametrize("T", PRECISIONS)
def test_the_one_call_form_is_the_single_one_call_per_view(rtw, T, denoise, gamma):
    """rtw_render_lens_batch_* on scene_2_spheres through three cameras with their apertures, 96 x 54 at 2 spp (the frame of the single
    one-call test), plain and filtered, gamma 0 (max_radius 16) and 1 (max_radius 32), per-view seeds: view v is on the bits
    rtw_render_wide_aperture_* with cams[v] and seeds[v], and the chain of the single calls on the pinhole copy; view 1 carries an explicit
    lens and a focus override, the others the camera's own (-1); rtw_stats() reports the render.  The cameras keep the single test's
    assumption -- some pixels beyond 8 px -- which the witness's CoC plane confirms here on the CPU"""
    import dataclasses
    cams = _cameras(rtw, T)
    scene = rtw.scene_2_spheres(elem_type=T)
    W, spp, mr, seeds = 96, 2, 32 if gamma else 16, [11, 12, 13]
    lens_radii, focus_dists = [-1.0, 0.55, -1.0], [0.0, 4.5, 0.0]          # (0.55: K is about 14 px, like the cameras' own)
    got = rtw.render_wide_aperture_batch(scene, cams, W, spp, seeds=seeds, denoise=denoise, device=0, gamma=gamma, wide_aperture=dict(max_radius=mr), lens_radii=lens_radii,
                                         focus_dists=focus_dists)
    st = rtw.last_stats()
    H = got.shape[1]
    assert got.shape == (3, H, W, 3) == (3, 54, 96, 3) and got.dtype == T and st["samples"] == 3 * W * H * spp
    for v, cam in enumerate(cams):
        lr = float(cam.lens_radius) if lens_radii[v] == -1 else lens_radii[v]
        single = rtw.render_wide_aperture(scene, cam, W, spp, seed=seeds[v], denoise=denoise, device=0, gamma=gamma,
                                          wide_aperture=dict(max_radius=mr, lens_radius=lens_radii[v], focus_dist=focus_dists[v]))
        _assert_same(got[v], single, f"view {v}: the single one-call form")
        pin = dataclasses.replace(cam, lens_radius=T(0))
        if denoise:
            linear = rtw.render_denoised(scene, pin, W, spp, seed=seeds[v], gamma=False, device=0, **denoise)
        else:
            linear = rtw.render(scene, pin, W, spp, seed=seeds[v], gamma=False, device=0)
        linear = np.ascontiguousarray(linear)
        feat = np.ascontiguousarray(rtw.render_features(scene, pin, W, spp, seed=seeds[v], device=0)["raw"])
        chain = rtw.wide_aperture(linear, feat, pin, gamma=gamma, device=0, lens_radius=lr, focus_dist=focus_dists[v], max_radius=mr)
        _assert_same(got[v], chain, f"view {v}: the chain of the single calls")
        plane = FO.coc_plane(linear, feat, pin, T, lr, focus_dists[v], mr)
        assert float(np.nanmax(plane[..., 0])) > 8, f"view {v}: no pixel beyond 8 px"
        if v == 0:
            wit_out, wit_work = WA.wide_aperture(linear, feat, pin, T, lens_radius=lr, focus_dist=focus_dists[v], max_radius=mr, gamma=int(gamma))
            assert (wit_work["lo_tile"] >= 0.5).any()
            _assert_same(got[v], wit_out, "view 0 against the witness")
