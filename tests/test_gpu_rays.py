"""Ray queries on the GPU (include/rtw_hip.h rtw_cast_rays_*) against the witness tests/rays_ref.py: per ray the oracle's
hit_world(scene, o, d, tmin, tmax_i) in the numerics mode that is current.  Every comparison is on the BITS -- the indices as they are, the
records viewed as unsigned integers.  Tolerance: NONE.

Every device buffer is sized for n rounded up to 256 plus a guard of 256 rays, pre-filled with -7; the words behind n are checked after
every call: the kernel writes nothing beyond n.  No test provokes a fault."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rays_ref as RR

pytestmark = pytest.mark.gpu

PRECISIONS = [np.float32, np.float64]
SCANS = {"matrix": 0, "valu": 4}          # RTW_FLAG_SCAN_VALU = 4
GUARD = 256
FILL = -7


def _sfx(T):
    return "f64" if np.dtype(T) == np.float64 else "f32"


def _stats(L):
    from rtw_amd import _capi
    st = _capi.Stats()
    _capi.check(L.rtw_stats(C.byref(st)))
    return st


def _padded(n):
    return (n + 255) // 256 * 256 + GUARD


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
        """-> device (rays, idx, rec), each padded and pre-filled with -7"""
        import torch
        n, m = rays.shape[0], _padded(rays.shape[0])
        host = np.full((m, 8), FILL, self.T)
        host[:n] = rays
        tdt = torch.float64 if self.T is np.float64 else torch.float32
        return (torch.from_numpy(host).to("cuda:0"), torch.full((m,), FILL, dtype=torch.int32, device="cuda:0"),
                torch.full((m * 8,), float(FILL), dtype=tdt, device="cuda:0"))

    def enqueue(self, bufs, n, flags=0, records=True, max_workgroups=0, stream=None, tmin=RR.TMIN):
        from rtw_amd import _capi, make_rays_params
        P = make_rays_params(tmin=tmin, flags=flags, max_workgroups=max_workgroups)
        d_rays, d_idx, d_rec = bufs
        fn = getattr(self.L, "rtw_cast_rays_device_" + _sfx(self.T))
        _capi.check(fn(self.handle, C.c_void_p(d_rays.data_ptr()), n, C.byref(P), C.c_void_p(d_idx.data_ptr()),
                       C.c_void_p(d_rec.data_ptr()) if records else None, C.c_void_p(stream) if stream else None))

    def fetch(self, bufs, n, records=True):
        """-> (idx [n], rec [n, 8]) after checking that nothing behind n (without records: nothing of the records at all) was written"""
        import torch
        torch.cuda.synchronize()
        idx, rec = bufs[1].cpu().numpy(), bufs[2].cpu().numpy().reshape(-1, 8)
        assert (idx[n:] == FILL).all() and idx[n:].size >= GUARD, "indices were written behind n"
        assert (rec[n if records else 0:] == FILL).all(), "records were written behind n"
        assert np.array_equal(bufs[0].cpu().numpy()[n:], np.full((idx.size - n, 8), FILL, self.T)), "the rays were written to"
        return idx[:n].copy(), rec[:n].copy()

    def cast(self, rays, **kw):
        """one call -> (idx, rec, stats)"""
        n, records = rays.shape[0], kw.get("records", True)
        bufs = self.buffers(rays)
        self.enqueue(bufs, n, **kw)
        st = _stats(self.L)
        idx, rec = self.fetch(bufs, n, records)
        return idx, rec, st


def _assert_same(idx, rec, ref_idx, ref_rec, what):
    bad = idx != ref_idx
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} indices differ from the oracle; first at {np.nonzero(bad)[0][:6].tolist()}: " \
                          f"{idx[bad][:6].tolist()} for {ref_idx[bad][:6].tolist()}"
    if rec is not None:
        assert rec.dtype == ref_rec.dtype and rec.shape == ref_rec.shape, what
        badr = RR.bits(rec) != RR.bits(ref_rec)
        assert not badr.any(), f"{what}: {int(badr.sum())} of {badr.size} record words differ from the oracle; first at {np.argwhere(badr)[:4].tolist()}"


def _assert_stats(st, n, n_spheres):
    assert st.samples == n and st.segments == n and st.sphere_tests == n * n_spheres and st.kernel_ms > 0
    assert st.block_threads == 256 and 1 <= st.grid_blocks <= (n + 255) // 256


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


# ---- instances ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
@pytest.mark.parametrize("name", RR.SCENES)
def test_every_population_equals_the_oracle(oracle, dev, name, T, scan):
    """all populations of a scene in one launch: the 485-sphere scene through the LDS instances, the 1600 / 800-sphere scenes through the
    global-memory ones, matrix pipe and RTW_FLAG_SCAN_VALU"""
    rays, ref_idx, ref_rec, where = RR.all_rays(name, T)
    ds = dev(name, T)
    idx, rec, st = ds.cast(rays, flags=SCANS[scan])
    for k, sl in where.items():
        _assert_same(idx[sl], rec[sl], ref_idx[sl], ref_rec[sl], f"{name} population {k}")
    _assert_stats(st, rays.shape[0], ds.n_spheres)
    if name == "dup":
        assert RR.DUP_SECOND in idx and RR.DUP_PAIR[1] in idx and RR.DUP_FIRST not in idx and RR.DUP_PAIR[0] not in idx


def test_group_cull_is_accepted_and_gives_the_same_words(oracle, dev):
    rays, ref_idx, ref_rec, _ = RR.all_rays("random", np.float32)
    idx, rec, _ = dev("random", np.float32).cast(rays, flags=1)
    _assert_same(idx, rec, ref_idx, ref_rec, "RTW_FLAG_GROUP_CULL")


@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["random", "big"])
def test_the_three_numerics_modes(oracle, dev, numerics, name, T, scan):
    """populations a, b and d in every numerics mode (the mode is a kernel argument): the witness and make_rays_params follow the fixture"""
    rays, ref_idx, ref_rec, where = RR.all_rays(name, T, which=("a", "b", "d"))
    idx, rec, _ = dev(name, T).cast(rays, flags=SCANS[scan])
    for k, sl in where.items():
        _assert_same(idx[sl], rec[sl], ref_idx[sl], ref_rec[sl], f"{numerics} {name} population {k}")


def far_scene(T):
    """coordinates of 2^41: beyond what the f16 split of the matrix-pipe filter covers (mf_ops null), so flags 0 runs the VALU instance"""
    c = np.array([[2.0 ** 41, 0, 0], [2.0 ** 41, 2.0 ** 39, 0], [0, 0, -5.0], [0, 2.0 ** 41, 2.0 ** 40]])
    r = np.array([2.0 ** 38, 2.0 ** 37, 1.0, 2.0 ** 39])
    z = np.zeros(4, T)
    flat = dict(n=4, cx=c[:, 0].astype(T), cy=c[:, 1].astype(T), cz=c[:, 2].astype(T), r=r.astype(T), kind=np.zeros(4, np.int32), ar=z + T(0.5), ag=z + T(0.5),
                ab=z + T(0.5), param=z)
    rng = np.random.default_rng(41)
    aim = np.concatenate([c, c + r[:, None] * rng.normal(size=(4, 3)) * 0.9, c + r[:, None] * rng.normal(size=(4, 3)) * 3.0, rng.normal(size=(12, 3))])
    d = aim / np.linalg.norm(aim, axis=1, keepdims=True)
    return flat, RR.pack(np.zeros_like(d), d, None, T)


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_a_scene_the_f16_split_cannot_cover_runs_the_valu_scan(oracle, T):
    flat, rays = far_scene(T)
    ref_idx, ref_rec = RR.expected(flat, rays, T)
    assert (ref_idx >= 0).sum() >= 6 and (ref_idx < 0).sum() >= 4 and len(set(ref_idx.tolist())) == 5
    with DeviceScene(flat, T) as ds:
        idx, rec, st = ds.cast(rays, flags=0)
        _assert_same(idx, rec, ref_idx, ref_rec, "2^41 scene")
        _assert_stats(st, rays.shape[0], 4)


_PROBE = """
import sys
sys.path[:0] = [{tests!r}, {root!r}, {oracle!r}]
import torch
torch.cuda.init()                       # (two HIP runtimes in one process: torch's goes first, tests/conftest.py)
import numpy as np
import test_gpu_rays as G
G.probe(np.{prec})
print("walked")
"""
PROBE_ROWS = [("random", 0, (1, 1)), ("random", 4, (1, 0)), ("random", 1, (1, 1)), ("big", 0, (0, 1)), ("big", 4, (0, 0)), ("far", 0, None)]     # (scene, flags, (lds_scene, mfma))


def probe(T):
    """one tiny launch per row of PROBE_ROWS (what the child process of the test below runs)"""
    import rtw_oracle
    rtw_oracle.build()
    for k, (name, flags, _) in enumerate(PROBE_ROWS):
        print("@row", k, file=sys.stderr, flush=True)
        flat, rays = far_scene(T) if name == "far" else (RR.scene(name, T)[0], RR.populations(name, T)["a"][:70])
        with DeviceScene(flat, T) as ds:
            ds.cast(rays, flags=flags)
            ds.cast(rays, flags=flags, records=False)


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_all_four_instances_of_a_precision_are_reached(T):
    """The environment aids are read once per process, so a fresh process per precision walks PROBE_ROWS under RTW_DEBUG: the launch reports
    the instance the row names -- together the four (lds_scene, mfma) instances of the precision, the 2^41 scene on the VALU scan under
    flags 0 -- and a grid that the ray count and the resident workgroups bound."""
    import re
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    code = _PROBE.format(tests=tests, root=root, oracle=os.path.join(root, "oracle"), prec=np.dtype(T).name)
    env = dict(os.environ, RTW_ENABLE_TEST_AIDS="1", RTW_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "walked" in r.stdout, r.stderr[-3000:]
    sections = r.stderr.split("@row ")[1:]
    assert len(sections) == len(PROBE_ROWS)
    pat = re.compile(r"\[rtw debug\] rays instance: (f32|f64) lds_scene=(\d) cull=0 mfma=(\d) records=(\d) lds_bytes=(\d+) blocks_per_cu=(\d+) grid=(\d+)\s*$", re.M)
    reached = set()
    for (name, flags, expect), text in zip(PROBE_ROWS, sections):
        lines = pat.findall(text)
        assert len(lines) == 2 and [int(ln[3]) for ln in lines] == [1, 0], (name, flags, text[-500:])
        for prec, lds, mfma, _, lds_bytes, per_cu, grid in lines:
            assert prec == _sfx(T) and int(lds_bytes) >= 8192 + 3072 and int(per_cu) >= 1 and int(grid) == 1, (name, flags, lines)
            if expect is None:
                assert int(mfma) == 0 and int(lds) == 1, (name, lines)
            else:
                assert (int(lds), int(mfma)) == expect, (name, flags, lines)
                reached.add((int(lds), int(mfma)))
    assert reached == {(0, 0), (0, 1), (1, 0), (1, 1)}


# ---- ray counts ---------------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)


@pytest.mark.parametrize("scan", SCANS)
@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_ray_counts_and_grid_caps(oracle, dev, T, scan):
    """the first n rays of the 485-sphere scene's populations, n around the wave and the workgroup size; n = 1000 with the grid capped at
    1 and 3 workgroups (every wave makes several trips, the last one ragged): the uncapped call's words"""
    rays, ref_idx, ref_rec, _ = RR.all_rays("random", T)
    ds = dev("random", T)
    for n in COUNTS:
        idx, rec, st = ds.cast(rays[:n], flags=SCANS[scan])
        _assert_same(idx, rec, ref_idx[:n], ref_rec[:n], f"n = {n}")
        _assert_stats(st, n, ds.n_spheres)
    for cap in (1, 3):
        capped_idx, capped_rec, st = ds.cast(rays[:1000], flags=SCANS[scan], max_workgroups=cap)
        assert st.grid_blocks == cap
        assert np.array_equal(capped_idx, idx) and np.array_equal(RR.bits(capped_rec), RR.bits(rec)), cap
        _assert_stats(st, 1000, ds.n_spheres)


# ---- other calls --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_without_records_the_indices_are_the_full_calls(oracle, dev, T):
    rays, ref_idx, _, _ = RR.all_rays("random", T)
    for flags in SCANS.values():
        idx, _, st = dev("random", T).cast(rays, flags=flags, records=False)
        _assert_same(idx, None, ref_idx, None, "rec == NULL")
        _assert_stats(st, rays.shape[0], dev("random", T).n_spheres)


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_the_host_form_equals_the_device_form(oracle, rtw, dev, T):
    flat = RR.scene("random", T)[0]
    rays, ref_idx, ref_rec, where = RR.all_rays("random", T)
    d_idx, d_rec, _ = dev("random", T).cast(rays)
    idx, rec = rtw.cast_rays(flat, rays, T=T)
    assert idx.dtype == np.int32 and rec.dtype == T and np.array_equal(idx, d_idx) and np.array_equal(RR.bits(rec), RR.bits(d_rec))
    st = rtw.last_stats()
    assert st["samples"] == st["segments"] == rays.shape[0] and st["sphere_tests"] == rays.shape[0] * flat["n"]
    _assert_same(idx, rec, ref_idx, ref_rec, "host form")
    # [n, 6]: tmax = inf, tag = 0 -- population (a) as it is; without records, under a cap and on the VALU scan
    a = where["a"]
    idx6, rec6 = rtw.cast_rays(flat, rays[a][:, :6], T=T)
    assert np.array_equal(idx6, d_idx[a]) and np.array_equal(RR.bits(rec6), RR.bits(d_rec[a]))
    idx_only, none = rtw.cast_rays(flat, rays, T=T, records=False, max_workgroups=2, flags=4)
    assert none is None and np.array_equal(idx_only, d_idx)


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_tags_change_nothing(oracle, dev, T):
    rays, ref_idx, ref_rec, _ = RR.all_rays("random", T, which=("a", "c", "e"))
    tagged = rays.copy()
    tagged[:, 7] = np.resize(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30, -7.0], T), rays.shape[0])
    for flags in SCANS.values():
        idx, rec, _ = dev("random", T).cast(tagged, flags=flags)
        _assert_same(idx, rec, ref_idx, ref_rec, "tagged rays")


def test_the_device_renderer_method_and_a_tmin_of_its_own(oracle, rtw, dev):
    """DeviceRenderer.cast_rays_into, and tmin = 0.5: one value per call, converted to T once -- the witness with that tmin"""
    import torch
    T = np.float32
    flat = RR.scene("random", T)[0]
    rays = RR.populations("random", T)["a"]
    n = rays.shape[0]
    ds = dev("random", T)
    bufs = ds.buffers(rays)
    dr = rtw.DeviceRenderer.__new__(rtw.DeviceRenderer)           # (the uploaded scene of the module: the method only needs handle, T and L)
    dr.T, dr.L, dr.handle = T, ds.L, ds.handle
    try:
        dr.cast_rays_into(bufs[0].data_ptr(), n, bufs[1].data_ptr(), bufs[2].data_ptr(), tmin=0.5)
        _stats(ds.L)
        idx, rec = ds.fetch(bufs, n)
    finally:
        dr.handle = C.c_void_p()                                   # (not this object's to free)
    ref_idx = np.empty(n, np.int32)
    ref_rec = np.zeros((n, 8), T)
    for i, ray in enumerate(rays):
        k, r = oracle.hit_world(flat, ray[0:3], ray[3:6], 0.5, float(ray[6]), T)
        ref_idx[i] = k
        if k >= 0:
            ref_rec[i] = r
    _assert_same(idx, rec, ref_idx, ref_rec, "tmin = 0.5")
    assert (rec[idx >= 0][:, 0] >= 0.5).all()
    torch.cuda.synchronize()


def test_a_handle_of_the_other_precision_or_device_is_refused(dev):
    ds = dev("random", np.float32)
    rays = RR.populations("random", np.float32)["a"]
    bufs = ds.buffers(rays)
    from rtw_amd import make_rays_params
    P = make_rays_params()
    args = (C.c_void_p(bufs[0].data_ptr()), 10, C.byref(P), C.c_void_p(bufs[1].data_ptr()), C.c_void_p(bufs[2].data_ptr()), None)
    assert ds.L.rtw_cast_rays_device_f64(ds.handle, *args) == -4 and b"precision" in ds.L.rtw_last_error()
    P.device = 5
    assert ds.L.rtw_cast_rays_device_f32(ds.handle, *args) == -4 and b"device" in ds.L.rtw_last_error()
    P.device = 0
    assert ds.L.rtw_cast_rays_device_f32(ds.handle, C.c_void_p(bufs[0].data_ptr()), 0, C.byref(P), C.c_void_p(bufs[1].data_ptr()), None, None) == 0       # n == 0: nothing enqueued
    import torch
    torch.cuda.synchronize()
    assert (bufs[1].cpu().numpy() == FILL).all() and (bufs[2].cpu().numpy() == FILL).all()


@pytest.mark.parametrize("T", PRECISIONS, ids=["f32", "f64"])
def test_two_calls_in_flight_on_two_streams(oracle, dev, T):
    import torch
    rays, ref_idx, ref_rec, _ = RR.all_rays("random", T)
    ds = dev("random", T)
    half = rays.shape[0] // 2
    parts = [(rays[:half], ref_idx[:half], ref_rec[:half], 0), (rays[half:], ref_idx[half:], ref_rec[half:], 4)]
    bufs = [ds.buffers(p[0]) for p in parts]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for _ in range(2):
        for b, p, s in zip(bufs, parts, streams):
            ds.enqueue(b, p[0].shape[0], flags=p[3], stream=s.cuda_stream)
    for b, p in zip(bufs, parts):
        idx, rec = ds.fetch(b, p[0].shape[0])
        _assert_same(idx, rec, p[1], p[2], f"stream with flags {p[3]}")
