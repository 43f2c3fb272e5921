"""Batched feature and filter passes on the GPU (include/rtw_hip.h rtw_render_features_batch_*, rtw_filter_batch_*,
rtw_render_filtered_batch_*).  No new arithmetic is defined, so the references are what they were: view v of a batched call against the
single-view device call on view v's inputs AND against the witnesses tests/features_ref.py / tests/denoise_ref.py applied view by view.
Every comparison is on the BITS; NaN pixels are compared as a set.  Tolerance: NONE.
That the filter inputs can tell a kernel whose taps cross a view's border from a right one is shown on the CPU: tests/test_filter_batch_ref.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import big_scenes as BS
import denoise_ref as DR
import features_ref as FR
import filter_batch_frames as FB
from conftest import CamObj
from test_gpu_denoise import DeviceFrame, _assert_same
from test_gpu_denoise import _params as denoise_params
from test_gpu_features import DeviceScene, _assert_same_bits, _stats

pytestmark = pytest.mark.gpu

SCAN_FLAGS = {"matrix": 0, "valu": 4}                  # RTW_FLAG_SCAN_VALU = 4
#: (W, H, views): 12 tiles per view (a multiple of a workgroup's 4 waves); 6 tiles (a workgroup's waves straddle a view border in the flat
#: numbering); one ragged tile per view
FEATURE_SHAPES = [(32, 18, 3), (24, 13, 3), (2, 1, 5)]
#: (spp, n_chunks, (chunk_begin, chunk_count)): all 4 one-sample chunks; s = 3, N = 2, the second (short, jittered) chunk alone
FEATURE_PARAMS = [(4, 4, (0, 4)), (5, 2, (1, 1))]


def _views(T, n):
    """the views of a feature batch: F's camera, t_cam2, F's camera again with another seed, ... -> [(camera dict, seed, cache key)]"""
    import rtw_amd
    _, cam_f, _, _ = FR.frame_f(T)
    cam2 = BS.camera_dict(rtw_amd.t_cam2(elem_type=T))
    cycle = [(cam_f, 1, "F"), (cam2, 1, "F-cam2"), (cam_f, 77, "F"), (cam2, 5, "F-cam2"), (cam_f, 1, "F")]
    return cycle[:n]


def features_batch_device(ds, views, W, H, spp, n_chunks, chunks, flags=0, seed=1, null_seeds=False):
    """rtw_render_features_batch_device_f32/_f64 on a test_gpu_features.DeviceScene -> (raw [N, H, W, 8], stats)"""
    from rtw_amd import _capi
    n = len(views)
    Cm = _capi.make_cameras([CamObj(v[0]) for v in views], ds.T)
    sd = None if null_seeds else _capi.make_seeds([v[1] for v in views], n)
    P = _capi.make_params(width=W, height=H, spp=spp, seed=seed, n_chunks=n_chunks, flags=flags)
    d = ds._buffer(n * W * H * 8)
    fn = ds.L.rtw_render_features_batch_device_f64 if ds.T is np.float64 else ds.L.rtw_render_features_batch_device_f32
    _capi.check(fn(ds.handle, Cm, n, sd, C.byref(P), chunks[0], chunks[1], C.c_void_p(d.data_ptr()), None))
    out, st = ds._fetch(d)
    return out.reshape(n, W, H, 8).transpose(0, 2, 1, 3), st


def features_batch_host(flat, views, T, W, H, spp, n_chunks, chunks, flags=0):
    """rtw_render_features_batch_f32/_f64 -> (raw [N, H, W, 8], stats)"""
    from rtw_amd import _capi
    L = _capi.lib()
    n = len(views)
    S, keep = _capi.make_scene(flat, T)
    Cm = _capi.make_cameras([CamObj(v[0]) for v in views], T)
    sd = _capi.make_seeds([v[1] for v in views], n)
    P = _capi.make_params(width=W, height=H, spp=spp, seed=1, n_chunks=n_chunks, flags=flags)
    out = np.full(n * W * H * 8, -7.0, T)
    fn = L.rtw_render_features_batch_f64 if T is np.float64 else L.rtw_render_features_batch_f32
    _capi.check(fn(C.byref(S), Cm, n, sd, C.byref(P), chunks[0], chunks[1], out.ctypes.data_as(C.c_void_p)))
    return out.reshape(n, W, H, 8).transpose(0, 2, 1, 3), _stats(L)


def _assert_batch_stats(st, n, W, H, count, n_spheres, N):
    assert st.samples == st.segments == n * W * H * count, (st.samples, st.segments)
    assert st.sphere_tests == st.segments * n_spheres
    assert st.n_chunks == N and st.kernel_ms > 0


# ---- features: the batch against the single-view device calls and the witness -----------------------------------------------------------
@pytest.mark.usefixtures("numerics")
@pytest.mark.parametrize("W,H,n", FEATURE_SHAPES)
@pytest.mark.parametrize("scan", ["matrix", "valu"])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_feature_views_equal_the_single_calls_and_the_witness(oracle, T, scan, W, H, n):
    flat = FR.frame_f(T)[0]
    views = _views(T, n)
    flags = SCAN_FLAGS[scan]
    with DeviceScene(flat, T) as ds:
        for spp, n_chunks, chunks in FEATURE_PARAMS:
            N = FR.effective_chunks(spp, n_chunks)[0]
            raw, st = features_batch_device(ds, views, W, H, spp, n_chunks, chunks, flags=flags)
            _assert_batch_stats(st, n, W, H, chunks[1], int(flat["n"]), N)
            for v, (cam, seed, key) in enumerate(views):
                what = f"{np.dtype(T).name} {scan} {W}x{H} spp {spp} chunks {chunks} view {v}"
                single, _ = ds.features(cam, W, H, spp, n_chunks, chunks, seed=seed, flags=flags)
                _assert_same_bits(np.ascontiguousarray(raw[v]), np.ascontiguousarray(single), what + " vs the single-view call")
                ref, poisoned = FR.resolve(FR.items(flat, cam, W, H, spp, n_chunks, seed, T, key=key), T, chunks)
                assert not poisoned.any()
                _assert_same_bits(np.ascontiguousarray(raw[v]), ref, what + " vs the witness")
            if n >= 3:
                assert not np.array_equal(FR.bits(raw[0]), FR.bits(raw[1]))                   # another camera
                if chunks[0] > 0:
                    assert not np.array_equal(FR.bits(raw[0]), FR.bits(raw[2]))               # the same camera, the view's own seed (jittered chunks)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_null_seeds_one_view_and_the_host_entry(oracle, T):
    flat = FR.frame_f(T)[0]
    views = _views(T, 3)
    W, H, spp, n_chunks, chunks = 24, 13, 5, 2, (0, 2)
    with DeviceScene(flat, T) as ds:
        # seeds == NULL: p->seed for every view
        raw, _ = features_batch_device(ds, views, W, H, spp, n_chunks, chunks, seed=9, null_seeds=True)
        named, _ = features_batch_device(ds, [(c, 9, k) for c, _, k in views], W, H, spp, n_chunks, chunks, seed=1)
        _assert_same_bits(np.ascontiguousarray(raw), np.ascontiguousarray(named), "seeds = NULL vs the seed named per view")
        for v, (cam, _, _) in enumerate(views):
            single, _ = ds.features(cam, W, H, spp, n_chunks, chunks, seed=9)
            _assert_same_bits(np.ascontiguousarray(raw[v]), np.ascontiguousarray(single), f"seeds = NULL, view {v}")
        # a batch of one view is the single-view call
        one, st = features_batch_device(ds, views[2:], W, H, spp, n_chunks, chunks)
        single, st1 = ds.features(views[2][0], W, H, spp, n_chunks, chunks, seed=views[2][1])
        _assert_same_bits(np.ascontiguousarray(one[0]), np.ascontiguousarray(single), "a batch of one view")
        assert (st.samples, st.segments, st.sphere_tests, st.n_chunks) == (st1.samples, st1.segments, st1.sphere_tests, st1.n_chunks)
        dev, _ = features_batch_device(ds, views, W, H, spp, n_chunks, chunks)
    host, st = features_batch_host(flat, views, T, W, H, spp, n_chunks, chunks)
    _assert_same_bits(np.ascontiguousarray(host), np.ascontiguousarray(dev), "host vs device entry point")
    _assert_batch_stats(st, 3, W, H, 2, int(flat["n"]), 2)
    host_valu, _ = features_batch_host(flat, views, T, W, H, spp, n_chunks, chunks, flags=SCAN_FLAGS["valu"] | 1)      # (group cull is accepted)
    _assert_same_bits(np.ascontiguousarray(host_valu), np.ascontiguousarray(dev), "host, VALU scan + group cull")


@pytest.mark.parametrize("scan", ["matrix", "valu"])
def test_a_global_scene_batch_equals_the_single_calls(scan):
    """1600 Float32 spheres (tests/big_scenes.py: more than the LDS copy holds), 8 x 5 pixels, 2 views"""
    T = np.float32
    flat = BS.scene(T)
    assert int(flat["n"]) == BS.BIG[T] == 1600
    cams = [BS.camera_dict(c) for c in BS.cameras(T)[:2]]
    views = [(cams[0], BS.VIEW_SEEDS[0], None), (cams[1], BS.VIEW_SEEDS[1], None)]
    with DeviceScene(flat, T) as ds:
        raw, st = features_batch_device(ds, views, 8, 5, 2, 2, (0, 2), flags=SCAN_FLAGS[scan])
        _assert_batch_stats(st, 2, 8, 5, 2, 1600, 2)
        for v, (cam, seed, _) in enumerate(views):
            single, _ = ds.features(cam, 8, 5, 2, 2, (0, 2), seed=seed, flags=SCAN_FLAGS[scan])
            _assert_same_bits(np.ascontiguousarray(raw[v]), np.ascontiguousarray(single), f"global scene {scan} view {v}")
        assert (raw[..., 7] > 0).any()


_PROBE = """
import sys
sys.path[:0] = [{tests!r}, {root!r}, {oracle!r}]
import torch
torch.cuda.init()                       # (two HIP runtimes in one process: torch's goes first, tests/conftest.py)
import numpy as np
import big_scenes as BS
import features_ref as FR
import test_gpu_filter_batch as TB
from test_gpu_features import DeviceScene
T = np.float32
for flat, views in ((FR.frame_f(T)[0], TB._views(T, 2)), (BS.scene(T), [(BS.camera_dict(c), 3, None) for c in BS.cameras(T)[:2]])):
    with DeviceScene(flat, T) as ds:
        for flags in (0, 4):
            TB.features_batch_device(ds, views, 8, 5, 2, 2, (0, 2), flags=flags)
        ds.features(views[0][0], 8, 5, 2, 2, (0, 2))
print("walked")
"""


def test_the_debug_line_of_a_batched_feature_launch_says_batch_1():
    """The environment aids are read once per process, so a fresh process launches under RTW_DEBUG: the batched launches report batch=1
    (scene in LDS and in global memory, both scans, the headline instance with its numerics fixed), the single-view call batch=0."""
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    env = dict(os.environ, RTW_ENABLE_TEST_AIDS="1", RTW_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", _PROBE.format(tests=tests, root=root, oracle=os.path.join(root, "oracle"))], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "walked" in r.stdout
    lines = [inst for inst, _, _ in BS.parse_instance_lines(r.stderr) if inst.kernel == "features"]
    I = BS.Instance
    assert lines == [I("features", "f32", 1, 0, 1, 1, 1, 0, 0), I("features", "f32", 1, 0, 0, 0, 1, 0, 0), I("features", "f32", 1, 0, 1, 1, 0, 0, 0),
                     I("features", "f32", 0, 0, 1, 0, 1, 0, 0), I("features", "f32", 0, 0, 0, 0, 1, 0, 0), I("features", "f32", 0, 0, 1, 0, 0, 0, 0)], lines


def test_a_scene_of_the_other_precision_is_refused():
    import torch
    from rtw_amd import _capi
    flat = FR.frame_f(np.float32)[0]
    views = _views(np.float64, 2)
    with DeviceScene(flat, np.float32) as ds:
        Cm = _capi.make_cameras([CamObj(v[0]) for v in views], np.float64)
        P = _capi.make_params(width=32, height=18, spp=4)
        d = torch.zeros(2 * 32 * 18 * 8, dtype=torch.float64, device="cuda:0")
        assert ds.L.rtw_render_features_batch_device_f64(ds.handle, Cm, 2, None, C.byref(P), 0, 4, C.c_void_p(d.data_ptr()), None) == -4
        assert b"precision" in ds.L.rtw_last_error()


# ---- filter: the batch against the single-view device call and the witness ---------------------------------------------------------------
class DeviceBatch:
    """a batch's inputs (tests/filter_batch_frames.py) as torch tensors on cuda:0, and the batched device entry point on them"""

    def __init__(self, N, W, H, T):
        import torch
        from rtw_amd import _capi
        self.L, self.T, self.N, self.W, self.H = _capi.lib(), T, N, W, H
        self.images, self.feats = FB.views(N, W, H, T)
        self.img = torch.from_numpy(FB.lib_layout(self.images)).to("cuda:0")
        self.feat = torch.from_numpy(FB.lib_layout(self.feats)).to("cuda:0")
        self.work_bytes = N * int(self.L.rtw_denoise_work_bytes(W, H, np.dtype(T).itemsize))
        torch.cuda.synchronize()

    def workspace(self, poison=False):
        import torch
        w = torch.zeros(self.work_bytes // np.dtype(self.T).itemsize, dtype=self.img.dtype, device="cuda:0")
        if poison:
            w.fill_(float("nan"))
        return w

    def run(self, work=None, stream=None, **kw):
        """-> the output tensor (not synchronised when a stream is given)"""
        import torch
        from rtw_amd import _capi
        work = self.workspace() if work is None else work
        out = torch.full((self.N * self.W * self.H * 3,), -7.0, dtype=self.img.dtype, device="cuda:0")
        torch.cuda.synchronize()                                   # the fills above ran on torch's stream
        D = denoise_params(**kw)
        fn = self.L.rtw_filter_batch_device_f64 if self.T is np.float64 else self.L.rtw_filter_batch_device_f32
        _capi.check(fn(C.byref(D), self.W, self.H, self.N, C.c_void_p(self.img.data_ptr()), C.c_void_p(self.feat.data_ptr()), C.c_void_p(out.data_ptr()),
                       C.c_void_p(work.data_ptr()), C.c_void_p(stream.cuda_stream) if stream is not None else None))
        self._keep = work
        if stream is None:
            torch.cuda.synchronize()
        return out

    def frames(self, out):
        return out.cpu().numpy().reshape(self.N, self.W, self.H, 3).transpose(0, 2, 1, 3)


def filter_batch_host(images, feats, T, **kw):
    """rtw_filter_batch_f32/_f64 -> [N, H, W, 3]"""
    from rtw_amd import _capi
    L = _capi.lib()
    N, H, W = images.shape[:3]
    img, f = FB.lib_layout(images), FB.lib_layout(feats)
    out = np.full(N * W * H * 3, -7.0, T)
    D = denoise_params(**kw)
    fn = L.rtw_filter_batch_f64 if T is np.float64 else L.rtw_filter_batch_f32
    _capi.check(fn(C.byref(D), W, H, N, img.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out.reshape(N, W, H, 3).transpose(0, 2, 1, 3)


def _assert_views(got, ref, what):
    assert got.shape == ref.shape, what
    for v in range(ref.shape[0]):
        _assert_same(got[v], ref[v], f"{what} view {v}")


@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("N,W,H,levels", FB.FILTER_FRAMES)
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_filter_views_equal_the_single_calls_and_the_witness(T, N, W, H, levels, entry):
    images, feats = FB.views(N, W, H, T)
    i, j = FB.nan_pixel(W, H)
    assert np.isnan(images[FB.NAN_VIEW, i, j]).any() and j == W - 1
    dev = DeviceBatch(N, W, H, T) if entry == "device" else None
    work = dev.workspace() if dev else None
    singles = [DeviceFrame(images[v], feats[v], T) for v in range(N)] if dev else None
    for m in (0, 1, 7):
        for demodulate in (True, False):
            for gamma in (0, 1):
                kw = dict(levels=levels, m=m, demodulate=demodulate, gamma=gamma)
                what = f"{np.dtype(T).name} {N} x {W}x{H} {entry} {kw}"
                got = dev.frames(dev.run(work=work, **kw)) if dev else filter_batch_host(images, feats, T, **kw)
                _assert_views(got, FB.witness(N, W, H, T, levels, m, demodulate, gamma), what + " vs the witness")
                assert np.isnan(got[FB.NAN_VIEW, i, j]).all()
                if dev:
                    single = np.stack([s.image(s.run(**kw)) for s in singles])
                    _assert_views(got, single, what + " vs the single-view device call")


@pytest.mark.parametrize("N,W,H,levels", FB.FILTER_FRAMES[2:])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_a_poisoned_workspace_and_two_streams(T, N, W, H, levels):
    import torch
    dev = DeviceBatch(N, W, H, T)
    ref = FB.witness(N, W, H, T, levels, 1, True, 1)
    _assert_views(dev.frames(dev.run(work=dev.workspace(poison=True), levels=levels)), ref, "a workspace full of NaN")
    for lv in (1, 2):                                               # (an odd and an even number of ping-pong steps)
        _assert_views(dev.frames(dev.run(work=dev.workspace(poison=True), levels=lv)), FB.witness(N, W, H, T, lv, 1, True, 1), f"poisoned, levels={lv}")
    wa, wb = dev.workspace(), dev.workspace(poison=True)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    oa = dev.run(work=wa, stream=sa, levels=levels)
    ob = dev.run(work=wb, stream=sb, levels=levels)
    sa.synchronize()
    sb.synchronize()
    _assert_views(dev.frames(oa), ref, "stream a")
    _assert_views(dev.frames(ob), ref, "stream b")


def test_the_profile_lines_of_a_batched_filter_carry_the_views():
    """RTW_DENOISE_PROFILE is read once per process: a fresh one runs one batched and one single-frame filter"""
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    code = ("import sys\nsys.path[:0] = [%r, %r, %r]\nimport torch\ntorch.cuda.init()\nimport numpy as np\nimport test_gpu_filter_batch as TB\n"
            "import filter_batch_frames as FB\nfrom test_gpu_denoise import DeviceFrame\n"
            "TB.DeviceBatch(3, 37, 23, np.float32).run(levels=2)\nim, ft = FB.views(3, 37, 23, np.float32)\nDeviceFrame(im[1], ft[1], np.float32).run(levels=2)\nprint('ran')\n"
            % (tests, root, os.path.join(root, "oracle")))
    env = dict(os.environ, RTW_ENABLE_TEST_AIDS="1", RTW_DENOISE_PROFILE="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "ran" in r.stdout, r.stderr[-3000:]
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("[rtw denoise]")]
    assert len(lines) == 8, lines                                   # prepare, 2 levels, total -- twice
    assert all(" 37x23 views=3 " in ln for ln in lines[:4]) and not any("views=" in ln for ln in lines[4:])
    assert "prepare" in lines[0] and "step=1 final=0" in lines[1] and "step=2 final=1" in lines[2] and "total levels=2" in lines[3]


# ---- one call: render, features, filter ----------------------------------------------------------------------------------------------------
def _render_batch_linear(flat, views, T, W, H, spp, n_chunks):
    """rtw_render_batch_f32/_f64 with gamma = 0 -> [N, H, W, 3]"""
    from rtw_amd import _capi
    L = _capi.lib()
    n = len(views)
    S, keep = _capi.make_scene(flat, T)
    Cm = _capi.make_cameras([CamObj(v[0]) for v in views], T)
    sd = _capi.make_seeds([v[1] for v in views], n)
    P = _capi.make_params(width=W, height=H, spp=spp, seed=1, n_chunks=n_chunks, gamma=0)
    out = np.empty(n * W * H * 3, T)
    fn = L.rtw_render_batch_f64 if T is np.float64 else L.rtw_render_batch_f32
    _capi.check(fn(C.byref(S), Cm, n, sd, C.byref(P), out.ctypes.data_as(C.c_void_p)))
    return out.reshape(n, W, H, 3).transpose(0, 2, 1, 3), _stats(L)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_render_filtered_batch_equals_render_denoised_view_by_view_and_the_witness(T):
    """frame F (32 x 18, 4 spp in 4 chunks), 3 views"""
    from rtw_amd import _capi
    flat, _, W, H = FR.frame_f(T)
    views = _views(T, 3)
    lin, render_st = _render_batch_linear(flat, views, T, W, H, 4, 4)
    raw, _ = features_batch_host(flat, views, T, W, H, 4, 4, (0, 4))
    L = _capi.lib()
    S, keep = _capi.make_scene(flat, T)
    Cm = _capi.make_cameras([CamObj(v[0]) for v in views], T)
    sd = _capi.make_seeds([v[1] for v in views], 3)
    fn = L.rtw_render_filtered_batch_f64 if T is np.float64 else L.rtw_render_filtered_batch_f32
    one = L.rtw_render_denoised_f64 if T is np.float64 else L.rtw_render_denoised_f32
    for gamma, kw in ((1, dict()), (0, dict(levels=2, m=3, demodulate=False))):
        P = _capi.make_params(width=W, height=H, spp=4, seed=1, n_chunks=4, gamma=gamma)
        D = denoise_params(gamma=1 - gamma, **kw)                    # d->gamma is replaced by p->gamma
        out = np.full(3 * W * H * 3, -7.0, T)
        _capi.check(fn(C.byref(S), Cm, 3, sd, C.byref(P), C.byref(D), out.ctypes.data_as(C.c_void_p)))
        st = _stats(L)
        got = out.reshape(3, W, H, 3).transpose(0, 2, 1, 3)
        # rtw_stats reports the batched render's record
        assert (st.samples, st.segments, st.n_chunks) == (render_st.samples, render_st.segments, render_st.n_chunks) and st.samples == 3 * W * H * 4
        assert st.segments > st.samples and st.kernel_ms > 0
        for v, (cam, seed, _) in enumerate(views):
            P1 = _capi.make_params(width=W, height=H, spp=4, seed=seed, n_chunks=4, gamma=gamma)
            Cm1 = _capi.make_camera(CamObj(cam), T)
            out1 = np.full(W * H * 3, -7.0, T)
            _capi.check(one(C.byref(S), C.byref(Cm1), C.byref(P1), C.byref(D), out1.ctypes.data_as(C.c_void_p)))
            _assert_same(got[v], out1.reshape(W, H, 3).transpose(1, 0, 2), f"gamma={gamma} view {v} vs the single-view call")
            ref = DR.denoise(np.ascontiguousarray(lin[v]), np.ascontiguousarray(raw[v]), T, gamma=gamma, **kw)
            _assert_same(got[v], ref, f"gamma={gamma} view {v} vs the witness on the product's own batch image and features")
    del keep


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def test_python_layer(rtw):
    import torch
    T = np.float32
    scene = rtw.scene_2_spheres(elem_type=T)
    cams = [rtw.t_default_cam(elem_type=T), rtw.t_cam2(elem_type=T), rtw.t_default_cam(elem_type=T)]
    seeds = [3, 4, 5]
    fb = rtw.render_features_batch(scene, cams, 24, 5, n_chunks=2, seeds=seeds)
    assert fb["raw"].shape == (3, 13, 24, 8) and fb["albedo"].shape == (3, 13, 24, 3) and fb["depth"].shape == fb["coverage"].shape == (3, 13, 24)
    assert fb["raw"].dtype == T and rtw.last_stats()["segments"] == 3 * 24 * 13 * 2
    for v in range(3):
        f1 = rtw.render_features(scene, cams[v], 24, 5, n_chunks=2, seed=seeds[v])
        _assert_same_bits(np.ascontiguousarray(fb["raw"][v]), np.ascontiguousarray(f1["raw"]), f"render_features_batch view {v}")
    dr = rtw.DeviceRenderer(scene, cams[0], device=0)
    try:
        d = torch.zeros(3 * 24 * 13 * 8, dtype=torch.float32, device="cuda:0")
        assert dr.features_batch_into(d.data_ptr(), cams, 24, 5, n_chunks=2, seeds=seeds, chunks=(1, 1), n_elems=d.numel()) == 13
        st = dr.stats()
        torch.cuda.synchronize()
        assert st["segments"] == 3 * 24 * 13
        part = rtw.render_features_batch(scene, cams, 24, 5, n_chunks=2, seeds=seeds, chunks=(1, 1))
        _assert_same_bits(np.ascontiguousarray(d.cpu().numpy().reshape(3, 24, 13, 8).transpose(0, 2, 1, 3)), np.ascontiguousarray(part["raw"]), "features_batch_into")
        with pytest.raises(ValueError):
            dr.features_batch_into(d.data_ptr(), cams, 24, 5, n_elems=24 * 13 * 8)
    finally:
        dr.close()
    # the filter: stacked arrays in, stacked arrays out; equal to the C calls and to denoise() view by view
    N, W, H, levels = FB.FILTER_FRAMES[2]
    images, feats = FB.views(N, W, H, T)
    got = rtw.denoise_batch(images, feats)
    assert got.shape == (N, H, W, 3) and got.dtype == T
    _assert_views(got, filter_batch_host(images, feats, T), "denoise_batch vs rtw_filter_batch_f32")
    _assert_views(got, np.stack([rtw.denoise(images[v], feats[v]) for v in range(N)]), "denoise_batch vs denoise")
    _assert_views(rtw.denoise_batch(images, dict(raw=feats), levels=2, normal_power_log2=7, demodulate=False, gamma=False),
                  FB.witness(N, W, H, T, 2, 7, False, 0), "denoise_batch keywords")
    dev = DeviceBatch(N, W, H, T)
    work, out = dev.workspace(), torch.zeros(N * W * H * 3, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rtw.denoise_batch_into(out.data_ptr(), dev.img.data_ptr(), dev.feat.data_ptr(), work.data_ptr(), W, H, N, elem_type=T, work_bytes=dev.work_bytes)
    torch.cuda.synchronize()
    _assert_views(dev.frames(out), got, "denoise_batch_into")
    # one call
    imgs = rtw.render_denoised_batch(scene, cams, 48, 4, seeds=seeds)
    assert imgs.shape == (3, 27, 48, 3) and imgs.dtype == T and rtw.last_stats()["samples"] == 3 * 48 * 27 * 4
    for v in range(3):
        _assert_same(imgs[v], rtw.render_denoised(scene, cams[v], 48, 4, seed=seeds[v]), f"render_denoised_batch view {v}")
    same_seed = rtw.render_denoised_batch(scene, cams[:2], 48, 4, seed=3)
    _assert_same(same_seed[0], imgs[0], "seed for every view")


# ---- the cached context across call kinds: one device buffer, one set of per-thread stats ---------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_call_kinds_share_the_cached_context_without_leaking_into_each_other(rtw, T):
    """Every host-buffer call goes through one cached context per device: ONE device buffer that each call kind sizes and partitions its own
    way (a frame, N frames, feature buffers, the denoiser's regions for one view or N) and ONE set of per-thread stats.  The eight calls
    below, made in one order and then in the reverse one, must each return the same bits both times -- so neither the buffer growing and
    shrinking between callers nor a previous caller's region offsets leak into a result -- and leave in last_stats() what their contract
    says: the render's record after a render + filter call, nothing new after a filter alone.
    40 x 22, 2 spp, depth 4, levels 3, 2 views: H is no multiple of 8 (partial tiles), 880 pixels are no multiple of 256, and the step 4
    taps cross the frame border.  Tolerance: NONE."""
    W, H, spp, n = 40, 22, 2, 2
    scene = rtw.scene_2_spheres(elem_type=T)
    cams = [rtw.t_default_cam(elem_type=T), rtw.t_cam2(elem_type=T)]
    seeds = [1, 9]
    kw = dict(depth=4)
    # the filter's inputs are the same arrays in both orders (made before either)
    image = np.ascontiguousarray(rtw.render(scene, cams[0], W, spp, gamma=False, **kw))
    feat = np.ascontiguousarray(rtw.render_features(scene, cams[0], W, spp)["raw"])
    images = np.ascontiguousarray(rtw.render_batch(scene, cams, W, spp, seed=seeds, gamma=False, **kw))
    feats = np.ascontiguousarray(rtw.render_features_batch(scene, cams, W, spp, seeds=seeds)["raw"])
    assert image.shape == (H, W, 3) and feats.shape == (n, H, W, 8)
    calls = [
        ("render", lambda: rtw.render(scene, cams[0], W, spp, **kw)),
        ("render_denoised_batch", lambda: rtw.render_denoised_batch(scene, cams, W, spp, seeds=seeds, levels=3, **kw)),
        ("render_features", lambda: rtw.render_features(scene, cams[1], W, spp, seed=9)["raw"]),
        ("denoise", lambda: rtw.denoise(image, feat, levels=3)),
        ("render_features_batch", lambda: rtw.render_features_batch(scene, cams, W, spp, seeds=seeds)["raw"]),
        ("denoise_batch", lambda: rtw.denoise_batch(images, feats, levels=3)),
        ("render_denoised", lambda: rtw.render_denoised(scene, cams[1], W, spp, seed=9, levels=3, **kw)),
        ("render (again)", lambda: rtw.render(scene, cams[0], W, spp, **kw)),
    ]
    shapes = {"render": (H, W, 3), "render_denoised_batch": (n, H, W, 3), "render_features": (H, W, 8), "denoise": (H, W, 3),
              "render_features_batch": (n, H, W, 8), "denoise_batch": (n, H, W, 3), "render_denoised": (H, W, 3), "render (again)": (H, W, 3)}

    def run(order):
        got = {}
        for name, call in order:
            before = dict(rtw.last_stats())
            res = call()
            st = rtw.last_stats()
            assert res.shape == shapes[name] and res.dtype == T, (name, res.shape, res.dtype)
            if name == "render_denoised":
                assert st["samples"] == W * H * spp, (name, st["samples"])
            elif name == "render_denoised_batch":
                assert st["samples"] == n * W * H * spp, (name, st["samples"])
            elif name in ("denoise", "denoise_batch"):
                assert st == before, f"{name} changed last_stats(): {before} -> {st}"
            got[name] = np.ascontiguousarray(res).tobytes()
        return got

    forward, backward = run(calls), run(calls[::-1])
    for name, _ in calls:
        assert forward[name] == backward[name], f"{name}: the result depends on the calls made before it"
    assert forward["render"] == forward["render (again)"] == backward["render (again)"]
