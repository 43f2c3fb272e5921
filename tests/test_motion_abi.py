"""Temporal reuse over moving spheres, CPU only (include/rtw_hip.h rtw_motion_table_*, rtw_first_hit_motion_*, rtw_animated_step_*): the
symbols are declared, listed and exported, the slot sizes are what the header says, the table is the witness's on the bits, and every refusal
of every new entry point is decided before any HIP call (the dummy device pointers below are never dereferenced)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import features_ref as FR
import motion_ref as MR
import temporal_ref as TR
from conftest import ROOT
from test_temporal_clamp_abi import BAD_C, _c
from test_temporal_noise_abi import BAD_SIZES, BAD_T, _has_gpu, _t

MOTION_SYMBOLS = ["rtw_motion_table_f32", "rtw_motion_table_f64", "rtw_first_hit_motion_device_f32", "rtw_first_hit_motion_device_f64", "rtw_first_hit_motion_f32",
                  "rtw_first_hit_motion_f64", "rtw_animated_step_device_f32", "rtw_animated_step_device_f64", "rtw_animated_step_f32", "rtw_animated_step_f64",
                  "rtw_render_animation_f32", "rtw_render_animation_f64"]
PY_NAMES = ["motion_table", "first_hit_motion", "first_hit_motion_into", "temporal_step_animated", "temporal_step_animated_into", "render_animation"]


@pytest.fixture(scope="module")
def lib(rtw):
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def test_symbols_declared_exported_and_listed(lib, rtw):
    import inspect
    from rtw_amd import _capi
    header = open(os.path.join(ROOT, "include", "rtw_hip.h")).read()
    declared = set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in MOTION_SYMBOLS:
        assert name in declared and name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, exported), name
    assert sorted(n for n in declared if "motion" in n or "animat" in n) == sorted(MOTION_SYMBOLS)
    assert lib.rtw_abi_version() == 4                    # additive: the ABI version stays
    for name in PY_NAMES:
        assert name in rtw.__all__ and callable(getattr(rtw, name)), name
    assert "d_motion_ptr" in inspect.signature(rtw.TemporalAccumulator.step).parameters
    # the temporal block no longer calls the scene static; the new block says what it leaves out
    assert "the scene is static" not in header
    block = header[header.index("Temporal reuse over moving spheres"):header.index("rtw_motion_table_f32(")]
    for word in ("Left out on purpose", "batched paths with motion", "motion blur", "the Julia shim", "LOWER caller's index"):
        assert word in block, word


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_table_is_the_witness_on_the_bits(lib, rtw, oracle, T):
    """rtw_motion_table_* (host code) and rtw.motion_table against motion_ref.motion_table: moved spheres, two new ones, one radius changed by an ulp"""
    from rtw_amd import _capi
    cur = {k: (np.asarray(v).copy() if isinstance(v, np.ndarray) else v) for k, v in FR.frame_f(T)[0].items()}
    n = int(cur["n"])
    prev = {k: (v[:n - 2].copy() if isinstance(v, np.ndarray) else n - 2) for k, v in cur.items()}
    rng = np.random.default_rng(4)
    for k in ("cx", "cy", "cz"):
        cur[k] = (cur[k].astype(np.float64) + rng.uniform(-0.3, 0.3, n)).astype(T)
    cur["r"][5] = np.nextafter(cur["r"][5], T(0))
    ref = MR.motion_table(prev, cur, T)
    got = rtw.motion_table(prev, cur, T)
    assert got.dtype == T and got.shape == (n, 4) and TR.same_bits(got, ref)
    assert np.isnan(got[[5, n - 2, n - 1], 0:3]).all() and np.isfinite(np.delete(got, [5, n - 2, n - 1], axis=0)).all() and (got[:, 3] == 0).all()
    fn = getattr(lib, "rtw_motion_table_" + ("f64" if T is np.float64 else "f32"))
    S, keep = _capi.make_scene(cur, T)
    tab = np.zeros((n, 4), T)
    assert fn(None, C.byref(S), tab.ctypes.data_as(C.c_void_p)) == -1 and fn(C.byref(S), None, tab.ctypes.data_as(C.c_void_p)) == -1 and fn(C.byref(S), C.byref(S), None) == -1
    assert fn(C.byref(S), C.byref(S), tab.ctypes.data_as(C.c_void_p)) == 0 and (tab == 0).all()      # a scene against itself: nothing moved
    del keep


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_motion_pass_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    dev, host = getattr(lib, "rtw_first_hit_motion_device_" + sfx), getattr(lib, "rtw_first_hit_motion_" + sfx)
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    err = lib.rtw_last_error
    W, H = 10, 6
    handle, tab, mo = 0x100000, 0x200000, 0x300000       # never dereferenced: every refusal below comes before the handle is looked at
    vp = lambda x: C.c_void_p(x) if x else None
    P = lambda **kw: _capi.make_params(kw.pop("w", W), kw.pop("h", H), kw.pop("spp", 1), **kw)

    def call(p=None, s=handle, c=cam, t=tab, m=mo, none=None):
        p = P() if p is None else p
        return dev(vp(s), None if c is None else C.byref(c), None if none == "p" else C.byref(p), vp(t), vp(m), None)

    assert call(none="p") == -1 and b"null" in err() and call(s=0) == -1 and call(c=None) == -1 and call(m=0) == -1
    for size, code in BAD_SIZES:
        p = P()
        p.width, p.height = size
        assert call(p) == code, size
    p = P()
    p.device = -2
    assert call(p) == -2
    for flags in (_capi.FLAG_COMPACT_TILES, _capi.FLAG_RAY_POOL, _capi.FLAG_RCCL_REDUCE, 64, 256, _capi.FLAG_NUMERICS_CONTRACT | 128):
        p = P()
        p.flags = flags
        assert call(p) == -2 and b"flags" in err(), flags
    # what the pass does not read is not checked: spp, depth, chunks
    p = P()
    p.spp, p.max_depth, p.n_chunks = 0, -5, -1
    assert call(p, m=0) == -1 and call(p, m=mo + 8) == -2 and b"aligned" in err() and call(p, t=tab + 4) == -2      # (it got past the parameters)
    # the host form: nulls, the same parameter checks, aliasing of the two host buffers
    flat = rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T)
    S, keep = _capi.make_scene(flat, T)
    out = np.zeros(W * H * 4 + int(S.n) * 4, T)
    o_ptr, t_ptr = out.ctypes.data, out.ctypes.data + W * H * 4 * eb
    hcall = lambda p=None, s=S, c=cam, t=t_ptr, m=o_ptr: host(None if s is None else C.byref(s), None if c is None else C.byref(c), None if p == "null" else C.byref(P() if p is None else p),
                                                           vp(t), vp(m))
    assert hcall(p="null") == -1 and hcall(s=None) == -1 and hcall(c=None) == -1 and hcall(m=0) == -1
    for size, code in BAD_SIZES:
        p = P()
        p.width, p.height = size
        assert hcall(p) == code, size
    assert hcall(t=o_ptr + 16) == -2 and b"alias" in err()
    if not _has_gpu():
        assert hcall() not in (0, -1, -2, -4, -5) and hcall(t=0) not in (0, -1, -2, -4, -5)       # everything in order: only the device is missing
    del keep


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_animated_step_is_refused_without_a_device(lib, rtw, T):
    """rtw_animated_step_device_*: everything the plain and the clamped step refuse, and the motion plane's own rules"""
    from rtw_amd import _capi
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_animated_step_device_" + sfx)
    W, H = 10, 6
    n_img, n_st, n_mo, n_mv = W * H * 3 * eb, lib.rtw_temporal_state_bytes(W, H, eb), lib.rtw_history_moment_bytes(W, H, eb), W * H * 4 * eb
    img, feat, sp, sn, out, mp, mn, mv = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000, 0x800000       # never dereferenced
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    err = lib.rtw_last_error
    vp = lambda x: C.c_void_p(x) if x else None

    def call(t=None, k="none", size=(W, H), c=cam, cp=cam, i=img, f=feat, v=mv, p=sp, q=mp, n=sn, m=mn, o=out, none=None):
        t = _t() if t is None else t
        ref = lambda x: None if x is None else C.byref(x)
        return fn(None if none == "t" else C.byref(t), None if k == "none" else C.byref(k), ref(c), ref(cp), *size, vp(i), vp(f), vp(v), vp(p), vp(n), vp(q), vp(m), vp(o), None)

    assert call(none="t") == -1 and b"null" in err()
    assert call(c=None) == -1 and call(i=0) == -1 and call(f=0) == -1 and call(n=0) == -1 and call(o=0) == -1 and call(m=0) == -1
    for bad in BAD_C:
        assert call(k=_c(**bad)) == -2 and b"clamp" in err(), bad
    for bad in BAD_T:
        assert call(_t(**bad)) == -2, bad
        assert call(_t(**bad), k=_c()) == -2, bad
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    # the motion plane: there exactly when the previous state is, aligned, no alias of an output
    assert call(v=0) == -2 and b"d_motion" in err() and call(v=0, k=_c()) == -2 and call(v=0, q=0, m=0) == -2
    assert call(cp=None, p=0, q=0) == -2 and b"d_motion" in err()                                     # a plane on the first frame
    assert call(v=mv + 8) == -2 and b"aligned" in err() and call(v=mv + 4, q=0, m=0) == -2
    assert call(v=out) == -2 and b"alias" in err() and call(v=sn + n_st - 16) == -2 and call(v=mn) == -2 and call(o=mv + n_mv - eb) == -2 and call(n=mv + 16) == -2
    # the rules of the underlying steps
    assert call(cp=None) == -2 and b"both" in err() and call(p=0) == -2
    assert call(q=0) == -2 and b"d_moment_prev" in err()
    assert call(f=feat + 8) == -2 and call(p=sp + 8) == -2 and call(n=sn + 8) == -2 and call(q=mp + 8) == -2 and call(i=img + 2) == -2
    assert call(o=sn) == -2 and b"alias" in err() and call(o=img + n_img - eb) == -2 and call(n=sp) == -2 and call(m=mp) == -2
    assert call(_t(gamma=9), o=0) == -1                 # precedence: a null beats a bad parameter
    if not _has_gpu():
        rc = call()                                     # everything in order: only the device is missing
        assert rc not in (0, -1, -2, -5)
        assert call(q=0, m=0) == rc and call(k=_c()) == rc and call(k=_c(radius=3, flags=1), q=0, m=0) == rc
        assert call(cp=None, p=0, q=0, v=0) == rc and call(cp=None, p=0, q=0, m=0, v=0) == rc        # the first frame is legal, with and without moments


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_host_step_is_refused_without_a_device(lib, rtw, T):
    from rtw_amd import _capi
    sfx, eb = ("f64", 8) if T is np.float64 else ("f32", 4)
    fn = getattr(lib, "rtw_animated_step_" + sfx)
    W, H = 10, 6
    n, ns, nm = W * H, lib.rtw_temporal_state_bytes(W, H, eb) // eb, lib.rtw_history_moment_bytes(W, H, eb) // eb
    sizes = dict(i=n * 3, f=n * 8, v=n * 4, o=n * 3, p=ns, nx=ns, q=nm, m=nm)
    buf = np.zeros(sum(sizes.values()) + 8, T)
    at, k = {}, 0
    for name, sz in sizes.items():
        at[name] = buf.ctypes.data + k * eb
        k += sz
    cam = _capi.make_camera(rtw.t_default_cam(elem_type=T), T)
    err = lib.rtw_last_error
    vp = lambda x: C.c_void_p(x) if x else None

    def call(t=None, k="none", size=(W, H), c=cam, cp=cam, none=None, **ptr):
        a = dict(at)
        a.update(ptr)
        t = _t() if t is None else t
        ref = lambda x: None if x is None else C.byref(x)
        return fn(None if none == "t" else C.byref(t), None if k == "none" else C.byref(k), ref(c), ref(cp), *size, vp(a["i"]), vp(a["f"]), vp(a["v"]), vp(a["p"]), vp(a["nx"]),
                  vp(a["q"]), vp(a["m"]), vp(a["o"]))

    assert call(none="t") == -1 and call(c=None) == -1 and call(i=0) == -1 and call(f=0) == -1 and call(nx=0) == -1 and call(o=0) == -1 and call(m=0) == -1
    for bad in BAD_T:
        assert call(_t(**bad)) == -2, bad
    for bad in BAD_C:
        assert call(k=_c(**bad)) == -2, bad
    for size, code in BAD_SIZES:
        assert call(size=size) == code, size
    assert call(v=0) == -2 and b"motion" in err() and call(cp=None, p=0, q=0) == -2 and b"motion" in err()
    assert call(cp=None) == -2 and call(p=0) == -2 and call(q=0) == -2
    assert call(o=at["v"]) == -2 and b"alias" in err() and call(nx=at["v"] + 16) == -2 and call(m=at["v"]) == -2 and call(o=at["i"]) == -2
    if not _has_gpu():
        rc = call()
        assert rc not in (0, -1, -2, -5)
        assert call(q=0, m=0) == rc and call(k=_c()) == rc and call(cp=None, p=0, q=0, v=0) == rc


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_animation_call_is_refused_without_a_device(lib, rtw, T):
    """rtw_render_animation_*: nulls, n_frames < 1, a bad scene of any frame, and everything rtw_render_sequence_* / rtw_render_path_clamped_*
    refuse of the params, the step, the clamp and the filter -- all before any HIP call"""
    from rtw_amd import _capi
    from rtw_amd.denoise import make_denoise
    sfx = "f64" if T is np.float64 else "f32"
    fn = getattr(lib, "rtw_render_animation_" + sfx)
    W, H, N = 10, 6, 3
    flat = rtw.flatten_scene(rtw.scene_2_spheres(elem_type=T), T)
    made = [_capi.make_scene(flat, T) for _ in range(N)]
    scenes = (type(made[0][0]) * N)(*[m[0] for m in made])
    cams = _capi.make_cameras([rtw.t_default_cam(elem_type=T)] * N, T)
    seeds = _capi.make_seeds(3, N)
    out = np.zeros(N * W * H * 3, T)
    err = lib.rtw_last_error
    P = lambda **kw: _capi.make_params(kw.pop("w", W), kw.pop("h", H), kw.pop("spp", 2), **kw)
    ref = lambda x: None if x is None else C.byref(x)

    def call(p="default", t="default", k=None, d=None, s=scenes, c=cams, n=N, sd=seeds, o=out.ctypes.data):
        return fn(s, c, n, sd, ref(P() if p == "default" else p), ref(_t() if t == "default" else t), ref(k), ref(d), C.c_void_p(o) if o else None)

    assert call(p=None) == -1 and b"null" in err() and call(t=None) == -1 and call(s=None) == -1 and call(c=None) == -1 and call(o=0) == -1
    for n in (0, -1, -7):
        assert call(n=n) == -2 and b"n_frames" in err(), n
    for bad in BAD_T:
        assert call(t=_t(**bad)) == -2, bad
    for bad in BAD_C:
        assert call(k=_c(**bad)) == -2, bad
    for size, code in BAD_SIZES:
        assert call(P(w=size[0], h=size[1])) == code, size
    assert call(P(spp=0)) == -2 and call(P(device=-2)) == -2 and call(P(flags=_capi.FLAG_COMPACT_TILES)) == -2 and call(P(shard_count=2)) == -2
    assert call(d=make_denoise(levels=0)) == -2
    # a bad scene in a LATER frame is found before anything runs: a negative count, a null array of a scene that has spheres
    for v in (0, N - 1):
        bad = (type(made[0][0]) * N)(*[m[0] for m in made])
        bad[v].n = -1
        assert call(s=bad) == -2 and b"sphere count" in err(), v
        bad[v].n = 2
        bad[v].r = None
        assert call(s=bad) == -1 and b"scene array" in err(), v
    if not _has_gpu():
        rc = call()
        assert rc not in (0, -1, -2, -4, -5)                  # everything in order: only the device is missing
        assert call(sd=None) == rc and call(k=_c()) == rc and call(d=make_denoise()) == rc and call(n=1) == rc
    del made


def test_c_animation_example_compiles_and_links(tmp_path):
    """examples/render_animation_c.c is plain C99 against include/rtw_hip.h and links against the built library"""
    from rtw_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "render_animation_c")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "render_animation_c.c"), "-L", lib_dir, "-lrtw_hip", f"-Wl,-rpath,{lib_dir}", "-lm",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not _has_gpu():
        r = subprocess.run([exe, "64", "2", "3"], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "no HIP device" in r.stderr
