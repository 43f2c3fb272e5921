"""Radiance queries on the GPU (include/rtw_hip.h rtw_trace_rays_*) against the witness tests/trace_rays_ref.py: per ray the exact sum of
the oracle's ray_color over its spp fresh streams, rounded once, divided by spp.  Every comparison is on the BITS (out viewed as uint64,
NaN matched as NaN).  Tolerance: NONE.

The device buffer of the results carries guard words filled with -7 on BOTH sides of out, checked after every call: the kernel writes
nothing outside its n x 3 values.  No test provokes a fault."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rays_ref as RR
import trace_rays_ref as TR

pytestmark = pytest.mark.gpu

PRECISIONS = [np.float32, np.float64]
SCANS = {"matrix": 0, "valu": 4}          # RTW_FLAG_SCAN_VALU = 4
GUARD = 96                                 # binary64 words on each side of out
FILL = -7.0


def _sfx(T):
    return "f64" if np.dtype(T) == np.float64 else "f32"


def _stats(L):
    from rtw_amd import _capi
    st = _capi.Stats()
    _capi.check(L.rtw_stats(C.byref(st)))
    return st


class DeviceScene:
    """an uploaded scene and the device-resident call on it"""

    def __init__(self, flat, T):
        from rtw_amd import _capi
        self.L, self.T, self.n_spheres = _capi.lib(), np.dtype(T).type, int(flat["n"])
        S, keep = _capi.make_scene(flat, T)
        self.handle = C.c_void_p()
        _capi.check(getattr(self.L, "rtw_scene_upload_" + _sfx(T))(C.byref(S), 0, C.byref(self.handle)))
        del keep

    def close(self):
        if self.handle:
            self.L.rtw_scene_free(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
        return False

    def buffers(self, rays):
        """-> device (rays: padded with -7 rows, out: GUARD words of -7, n x 3 words of -7, GUARD words of -7)"""
        import torch
        n = rays.shape[0]
        host = np.full((n + 64, 8), FILL, self.T)
        host[:n] = rays
        return torch.from_numpy(host).to("cuda:0"), torch.full((2 * GUARD + 3 * n,), FILL, dtype=torch.float64, device="cuda:0")

    def enqueue(self, bufs, n, *, spp, max_depth=16, flags=0, max_workgroups=0, stream=None, seed=TR.SEED, first_stream=0, first_sample=0, ray0=0):
        from rtw_amd import _capi, make_trace_params
        P = make_trace_params(spp=spp, max_depth=max_depth, seed=seed, first_stream=first_stream, first_sample=first_sample, flags=flags, max_workgroups=max_workgroups)
        d_rays, d_out = bufs
        fn = getattr(self.L, "rtw_trace_rays_device_" + _sfx(self.T))
        _capi.check(fn(self.handle, C.c_void_p(d_rays.data_ptr() + ray0 * 8 * d_rays.element_size()), n, C.byref(P),
                       C.c_void_p(d_out.data_ptr() + 8 * (GUARD + 3 * ray0)), C.c_void_p(stream) if stream else None))

    def fetch(self, bufs, n, rays=None):
        """-> out [n, 3] after checking the guard words on both sides and that the rays were not written to"""
        import torch
        torch.cuda.synchronize()
        w = bufs[1].cpu().numpy()
        assert w.size == 2 * GUARD + 3 * n
        assert (w[:GUARD] == FILL).all(), "words in front of out were written"
        assert (w[GUARD + 3 * n:] == FILL).all(), "words behind out were written"
        if rays is not None:
            back = bufs[0].cpu().numpy()
            assert np.array_equal(RR.bits(back[:n]), RR.bits(rays)) and (back[n:] == FILL).all(), "the rays were written to"
        return w[GUARD:GUARD + 3 * n].reshape(n, 3).copy()

    def trace(self, rays, **kw):
        """one call -> (out, stats)"""
        bufs = self.buffers(rays)
        self.enqueue(bufs, rays.shape[0], **kw)
        st = _stats(self.L)
        return self.fetch(bufs, rays.shape[0], rays), st


def _assert_same(out, ref, what):
    assert out.dtype == np.float64 and out.shape == ref.shape, what
    if not TR.same_words(out, ref):
        bad = ~((out.view(np.uint64) == ref.view(np.uint64)) | (np.isnan(out) & np.isnan(ref)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} words differ from the witness; first at {np.argwhere(bad)[:4].tolist()}: "
                             f"{out[bad][:4].tolist()} for {ref[bad][:4].tolist()}")


_scenes = {}


@pytest.fixture
def dev(request):
    """DeviceScene of (name, T), uploaded once per module"""
    def get(name, T):
        key = (name, np.dtype(T).name)
        if key not in _scenes:
            _scenes[key] = DeviceScene(RR.scene(name, T)[0], T)
        return _scenes[key]
    return get


@pytest.fixture(scope="module", autouse=True)
def _free_scenes():
    yield
    for ds in _scenes.values():
        ds.close()
    _scenes.clear()


# ---- against the witness ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
@pytest.mark.parametrize("name", TR.SMALL_SCENES)
def test_every_list_equals_the_witness(oracle, dev, name, T, scan):
    """primary, bounce and inside rays of a scene, spp 1, 2, 7 x max_depth 1, 2, 16, 50, matrix pipe and RTW_FLAG_SCAN_VALU; the stats of
    every call: samples = n spp, segments = the witness's count of scans with a live ray"""
    rays, where = TR.rays_of(name, T)
    ds = dev(name, T)
    n = rays.shape[0]
    for depth in TR.DEPTHS:
        for spp in TR.SPPS:
            out, st = ds.trace(rays, spp=spp, max_depth=depth, flags=SCANS[scan])
            ref = TR.expected(name, T, depth, spp)
            for k, sl in where.items():
                _assert_same(out[sl], ref[sl], f"{name} population {k} spp {spp} depth {depth}")
            segs = TR.segments_b(name, T, depth, spp)
            assert st.samples == n * spp and st.segments == segs and st.sphere_tests == segs * ds.n_spheres and st.kernel_ms > 0, (spp, depth, st.samples, st.segments, segs)
            assert st.block_threads == 256 and 1 <= st.grid_blocks <= (n + 255) // 256


@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_the_global_memory_instances_on_the_big_scene(oracle, dev, T, scan):
    rays = TR.big_rays(T)
    out, st = dev("big", T).trace(rays, spp=2, max_depth=16, flags=SCANS[scan])
    _assert_same(out, TR.expected("big", T, 16, 2), "big scene")
    assert st.samples == 2 * rays.shape[0]


def test_group_cull_is_accepted_and_gives_the_same_words(oracle, dev):
    rays, _ = TR.rays_of("random", np.float32)
    out, _ = dev("random", np.float32).trace(rays, spp=2, flags=1)
    _assert_same(out, TR.expected("random", np.float32, 16, 2), "RTW_FLAG_GROUP_CULL")


@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_the_three_numerics_modes(oracle, dev, numerics, T, scan):
    """the mode is a kernel argument: the witness and make_trace_params follow the fixture"""
    rays, _ = TR.rays_of("random", T)
    out, _ = dev("random", T).trace(rays, spp=2, max_depth=16, flags=SCANS[scan])
    _assert_same(out, TR.expected("random", T, 16, 2), f"{numerics}")


_PROBE = """
import sys
sys.path[:0] = [{tests!r}, {root!r}, {oracle!r}]
import torch
torch.cuda.init()                       # (two HIP runtimes in one process: torch's goes first, tests/conftest.py)
import numpy as np
import test_gpu_trace_rays as G
G.probe(np.{prec})
print("walked")
"""
PROBE_ROWS = [("random", 0, (1, 1)), ("random", 4, (1, 0)), ("random", 1, (1, 1)), ("big", 0, (0, 1)), ("big", 4, (0, 0))]     # (scene, flags, (lds_scene, mfma))


def probe(T):
    """one tiny launch per row of PROBE_ROWS (what the child process of the test below runs)"""
    import rtw_oracle
    rtw_oracle.build()
    for k, (name, flags, _) in enumerate(PROBE_ROWS):
        print("@row", k, file=sys.stderr, flush=True)
        with DeviceScene(RR.scene(name, T)[0], T) as ds:
            ds.trace(RR.populations(name, T)["a"][:70], spp=2, flags=flags)


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_all_four_instances_of_a_precision_are_reached(T):
    """The environment aids are read once per process, so a fresh process per precision walks PROBE_ROWS under RTW_DEBUG: the launch reports
    the instance the row names -- together the four (lds_scene, mfma) instances of the precision."""
    import re
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    code = _PROBE.format(tests=tests, root=root, oracle=os.path.join(root, "oracle"), prec=np.dtype(T).name)
    env = dict(os.environ, RTW_ENABLE_TEST_AIDS="1", RTW_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "walked" in r.stdout, r.stderr[-3000:]
    sections = r.stderr.split("@row ")[1:]
    assert len(sections) == len(PROBE_ROWS)
    pat = re.compile(r"\[rtw debug\] trace_rays instance: (f32|f64) lds_scene=(\d) cull=0 mfma=(\d) spp=(\d+) lds_bytes=(\d+) blocks_per_cu=(\d+) grid=(\d+)\s*$", re.M)
    reached = set()
    for (name, flags, expect), text in zip(PROBE_ROWS, sections):
        lines = pat.findall(text)
        assert len(lines) == 1, (name, flags, text[-500:])
        prec, lds, mfma, spp, lds_bytes, per_cu, grid = lines[0]
        assert prec == _sfx(T) and int(spp) == 2 and int(lds_bytes) >= 8192 + 3072 and int(per_cu) >= 1 and int(grid) == 1, (name, flags, lines)
        assert (int(lds), int(mfma)) == expect, (name, flags, lines)
        reached.add((int(lds), int(mfma)))
    assert reached == {(0, 0), (0, 1), (1, 0), (1, 1)}


# ---- the lane loop's edges ----------------------------------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 129, 257, 1000)
_edge = {}


def _edge_ref(T):
    key = np.dtype(T).name
    if key not in _edge:
        _edge[key] = TR.resolve(TR.sample_radiances(RR.scene("random", T)[0], TR.edge_rays(T), T, 16, 3))
    return _edge[key]


@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_ray_counts_and_grid_caps(oracle, dev, T, scan):
    """the first n rays of the edge list, n around the wave size and across batches, spp 3: the first and the last batch, the refill across a
    batch boundary, the empty lanes of the tail -- uncapped and with the grid capped at 1 and 3 workgroups"""
    rays, ref = TR.edge_rays(T), _edge_ref(T)
    ds = dev("random", T)
    for n in COUNTS:
        for cap in (0, 1, 3):
            out, st = ds.trace(rays[:n], spp=3, flags=SCANS[scan], max_workgroups=cap)
            _assert_same(out, ref[:n], f"n = {n} cap {cap}")
            assert st.samples == 3 * n and 1 <= st.grid_blocks <= (n + 255) // 256 and (not cap or st.grid_blocks == min(cap, (n + 255) // 256))


@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_a_long_path_among_primary_misses(oracle, dev, T, scan):
    """one ray inside the bubble (depth 50: some of its samples run out of depth) among rays that miss at once: its neighbours are refilled
    many times while it stays, and it keeps its sums across all of that"""
    flat = RR.scene("bubble", T)[0]
    ray, misses = TR.long_path_list(T)
    rays = np.concatenate([misses[:37], ray[None, :], misses[37:130]])
    ref = TR.resolve(TR.sample_radiances(flat, rays, T, 50, 7))
    assert not TR.same_words(ref[37], TR.sky(rays[37:38], T)[0])
    out, st = dev("bubble", T).trace(rays, spp=7, max_depth=50, flags=SCANS[scan])
    _assert_same(out, ref, "long path")
    assert st.samples == 7 * rays.shape[0] and st.segments > 7 * rays.shape[0] + 100


# ---- properties that need no oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_a_list_traced_in_two_calls(oracle, dev, T):
    """the second call with first_stream advanced by the first call's n: the words of the one call -- into one buffer, and the second call
    alone against the tail"""
    rays, _ = TR.rays_of("random", T)
    ds = dev("random", T)
    n, k = rays.shape[0], 77
    whole, _ = ds.trace(rays, spp=3, first_stream=1000)
    bufs = ds.buffers(rays)
    ds.enqueue(bufs, k, spp=3, first_stream=1000)
    ds.enqueue(bufs, n - k, spp=3, first_stream=1000 + k, ray0=k)
    _stats(ds.L)
    assert TR.same_words(ds.fetch(bufs, n, rays), whole)
    tail, _ = ds.trace(rays[k:], spp=3, first_stream=1000 + k)
    assert TR.same_words(tail, whole[k:])
    # a ray placed twice gets two independent estimates; the same stream gives the same one
    twice = np.concatenate([rays[:60], rays[:60]])
    out, _ = ds.trace(twice, spp=3, first_stream=1000)
    assert TR.same_words(out[:60], whole[:60]) and not TR.same_words(out[60:], whole[:60])
    again, _ = ds.trace(rays[:60], spp=3, first_stream=1060)
    assert TR.same_words(out[60:], again)


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_seed_and_first_sample_move_the_rays_that_scatter_only(oracle, dev, T):
    rays, _ = TR.rays_of("random", T)
    ds = dev("random", T)
    hit = RR.unbounded(RR.scene("random", T)[0], rays, T)[0] >= 0
    # the rays that MUST move: the first hit is a Lambertian sphere (a continuous draw whatever the stream) and the base sample reached the
    # sky, so its words are those of no other path.  (A ray that starts inside an opaque sphere is black on every stream; one that meets
    # only glass and polished metal draws a choice, not a direction: neither has to move.)
    diffuse = np.array([bool(row[0]["missed"] and row[0]["kinds"] and row[0]["kinds"][0] == 0) for row in TR.walks("random", T)])
    assert hit.sum() >= 50 and (~hit).sum() >= 10 and diffuse.sum() >= 40 and not (diffuse & ~hit).any()
    base, _ = ds.trace(rays, spp=1)
    sky = TR.sky(rays, T)
    assert TR.same_words(base[~hit], sky[~hit])
    for kw in (dict(first_sample=1), dict(seed=TR.SEED + 1), dict(first_stream=5)):
        out, _ = ds.trace(rays, spp=1, **kw)
        assert TR.same_words(out[~hit], sky[~hit]), kw
        moved = (out.view(np.uint64) != base.view(np.uint64)).any(axis=1)
        assert not moved[~hit].any() and moved[diffuse].all(), (kw, int(moved[diffuse].sum()), int(diffuse.sum()))
    # spp = 2 from first_sample 0 is the exact mean of the two spp = 1 calls
    two, _ = ds.trace(rays, spp=2)
    one, _ = ds.trace(rays, spp=1, first_sample=1)
    mean = np.array([[oracle.fx_sum([base[i, c], one[i, c]])[0] / 2.0 for c in range(3)] for i in range(rays.shape[0])])
    assert TR.same_words(two, mean)


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_depth_one_is_the_sky_where_the_ray_query_reports_a_miss(oracle, rtw, dev, T):
    flat = RR.scene("random", T)[0]
    rays, _ = TR.rays_of("random", T)
    idx, _ = rtw.cast_rays(flat, rays[:, :6], T=T, records=False)          # (unbounded: ray_color does not read tmax)
    out, st = dev("random", T).trace(rays, spp=3, max_depth=1)
    sky = TR.sky(rays, T)
    ref = np.array([[oracle.fx_sum([sky[i, c]] * 3)[0] / 3.0 if idx[i] < 0 else 0.0 for c in range(3)] for i in range(rays.shape[0])])
    assert (idx >= 0).any() and (idx < 0).any()
    _assert_same(out, ref, "max_depth = 1")
    assert not np.signbit(out[idx >= 0]).any()
    assert st.segments == 3 * rays.shape[0]
    for spp in (1, 2, 7):                       # max_depth 0: black without a scan, and without a loop over the samples
        black, st = dev("random", T).trace(rays, spp=spp, max_depth=0)
        assert (black.view(np.uint64) == 0).all() and st.segments == 0 and st.samples == spp * rays.shape[0], spp


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_the_host_form_equals_the_device_form(oracle, rtw, dev, T):
    flat = RR.scene("random", T)[0]
    rays, where = TR.rays_of("random", T)
    d_out, d_st = dev("random", T).trace(rays, spp=2, max_depth=16)
    out = rtw.trace_rays(flat, rays, spp=2, seed=TR.SEED, T=T)
    assert out.dtype == np.float64 and out.shape == (rays.shape[0], 3) and TR.same_words(out, d_out)
    st = rtw.last_stats()
    assert st["samples"] == 2 * rays.shape[0] and st["segments"] == d_st.segments and st["sphere_tests"] == d_st.segments * flat["n"]
    # [n, 6] rays, under a cap, on the VALU scan, with streams and samples of its own
    a = where["a"]
    d6, _ = dev("random", T).trace(rays[a], spp=3, max_depth=5, seed=9, first_stream=40, first_sample=2)
    out6 = rtw.trace_rays(flat, rays[a][:, :6], spp=3, max_depth=5, seed=9, first_stream=40, first_sample=2, T=T, max_workgroups=2, flags=4)
    assert TR.same_words(out6, d6)


def test_tmax_and_tag_are_not_read(oracle, dev):
    T = np.float32
    rays, _ = TR.rays_of("random", T)
    other = rays.copy()
    other[:, 6] = np.resize(np.array([0.0, 1e-6, np.nan, -1.0, np.inf], T), rays.shape[0])
    other[:, 7] = np.resize(np.array([np.nan, np.inf, -0.0, 1e30], T), rays.shape[0])
    a, _ = dev("random", T).trace(rays, spp=2)
    b, _ = dev("random", T).trace(other, spp=2)
    assert TR.same_words(a, b)


def test_the_device_renderer_method(oracle, rtw, dev):
    T = np.float32
    rays, _ = TR.rays_of("two", T)
    n = rays.shape[0]
    ds = dev("two", T)
    bufs = ds.buffers(rays)
    dr = rtw.DeviceRenderer.__new__(rtw.DeviceRenderer)           # (the uploaded scene of the module: the method only needs handle, T and L)
    dr.T, dr.L, dr.handle = T, ds.L, ds.handle
    try:
        dr.trace_rays_into(bufs[0].data_ptr(), n, bufs[1].data_ptr() + 8 * GUARD, spp=2, max_depth=16, seed=TR.SEED)
        _stats(ds.L)
        out = ds.fetch(bufs, n, rays)
    finally:
        dr.handle = C.c_void_p()                                   # (not this object's to free)
    _assert_same(out, TR.expected("two", T, 16, 2), "DeviceRenderer.trace_rays_into")


def test_a_handle_of_the_other_precision_or_device_is_refused(dev):
    ds = dev("random", np.float32)
    rays, _ = TR.rays_of("random", np.float32)
    bufs = ds.buffers(rays)
    from rtw_amd import make_trace_params
    P = make_trace_params(spp=1)
    args = (C.c_void_p(bufs[0].data_ptr()), 10, C.byref(P), C.c_void_p(bufs[1].data_ptr()), None)
    assert ds.L.rtw_trace_rays_device_f64(ds.handle, *args) == -4 and b"precision" in ds.L.rtw_last_error()
    P.device = 5
    assert ds.L.rtw_trace_rays_device_f32(ds.handle, *args) == -4 and b"device" in ds.L.rtw_last_error()
    P.device = 0
    assert ds.L.rtw_trace_rays_device_f32(ds.handle, C.c_void_p(bufs[0].data_ptr()), 0, C.byref(P), C.c_void_p(bufs[1].data_ptr()), None) == 0       # n == 0: nothing enqueued
    import torch
    torch.cuda.synchronize()
    assert (bufs[1].cpu().numpy() == FILL).all()


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_two_calls_in_flight_on_two_streams(oracle, dev, T):
    import torch
    rays, _ = TR.rays_of("random", T)
    ref = TR.expected("random", T, 16, 2)
    ds = dev("random", T)
    half = rays.shape[0] // 2
    parts = [(rays[:half], ref[:half], 0, 0), (rays[half:], ref[half:], 4, half)]
    bufs = [ds.buffers(p[0]) for p in parts]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for _ in range(2):
        for b, p, s in zip(bufs, parts, streams):
            ds.enqueue(b, p[0].shape[0], spp=2, flags=p[2], first_stream=p[3], stream=s.cuda_stream)
    for b, p in zip(bufs, parts):
        _assert_same(ds.fetch(b, p[0].shape[0], p[0]), p[1], f"stream with flags {p[2]}")


def test_c_example_runs(tmp_path):
    """examples/trace_rays_c.c: the probe prints its means and finds the list traced in two calls equal to the one call"""
    from conftest import ROOT
    from rtw_amd import _capi
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "trace_rays_c")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "trace_rays_c.c"),
                           "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0 and "traced in two calls: the same words" in r.stdout and "24576 samples" in r.stderr, (r.stdout, r.stderr)
    up = [float(x) for x in r.stdout.split("upper hemisphere: mean radiance (")[1].split(")")[0].split(",")]
    assert all(0.4 < x <= 1.0 for x in up) and up[2] >= up[0]          # the sky: white to blue, never above 1
