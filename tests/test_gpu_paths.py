"""The batched temporal steps on the GPU (include/rtw_hip.h rtw_reproject_batch_device_*, rtw_reproject_noise_batch_device_*,
rtw_render_paths_*) against the witness tests/paths_ref.py -- the single witnesses side by side -- and against the single device calls, path by
path.  Every comparison is on the BITS -- the image, the three planes of the state, the moment plane, the noise map; NaN values are compared as
a set.  Tolerance: NONE: a batched step has no arithmetic of its own.
Frames (W x H), S paths in {1, 3}: 1x1 and 5x3 (the whole batch is smaller than a wave); 37x23 (851 pixels: no multiple of 64 or 256, and odd, so
the strides between states and between moment planes carry 4 / 8 bytes of padding); 3x2, 9x33 and 70x40 (the clamped kernel's 32 x 8 tile: a
frame smaller than the window, tail tiles in both directions).  tests/test_paths_ref.py shows that these inputs reach the frame's edge -- where a
batched kernel that did not bound its taps would read the neighbouring path -- and every regime of the clamp and the noise map."""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_ref as DR
import paths_ref as PR
import temporal_noise_ref as NR
import temporal_ref as TR
from test_gpu_temporal_noise import _assert_same, _lib_layout, _nparams, _sfx, _tparams, _STAT_KEYS
from test_gpu_temporal_clamp import _cparams

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 3), (37, 23), (3, 2), (9, 33), (70, 40)]
TYPES = [np.float32, np.float64]
#: name -> (moments, clamp)
FORMS = {"plain": (False, None), "moments": (True, None), "clamped": (False, dict(PR.CLAMP)), "clamped+moments": (True, dict(PR.CLAMP)),
         "clamped+guides": (False, dict(PR.CLAMP, guides=True)), "clamped+guides+moments": (True, dict(PR.CLAMP, guides=True, radius=2))}
STEP_KW = dict(m=1)


@functools.lru_cache(maxsize=None)
def _inputs(size, T):
    """the hand-made inputs of the three paths at this size; read-only"""
    W, H = size
    inputs = [PR.path_inputs(H, W, T, s) for s in range(PR.N_PATHS)]
    for _, frames, st, mo, _ in inputs:
        for a in [x for f in frames for x in f] + list(st.values()) + [mo]:
            a.setflags(write=False)
    return inputs


@functools.lru_cache(maxsize=None)
def _chain(size, T, form, start):
    """the witness of three chained steps of every path -> [step][path] = (out, state, moment or None).  start: "first" (step 0 is a first
    frame) or "state" (step 0 runs on the hand-made previous states)"""
    inputs = _inputs(size, T)
    moments, clamp = FORMS[form]
    prev = None if start == "first" else [(st, mo if moments else None, c0) for (_, _, st, mo, c0) in inputs]
    steps = []
    for k in range(3):
        res = PR.step(inputs, k, T, prev, moments=moments, clamp=clamp, **STEP_KW)
        steps.append(res)
        prev = [(r[1], r[2], inputs[s][0][k]) for s, r in enumerate(res)]
    return steps


class PathFrames:
    """the frames of S paths, their hand-made previous states and moment planes as torch tensors on cuda:0 in the batched layouts, and the
    batched and the single device entry points on them"""

    def __init__(self, size, T, S):
        import torch
        import rtw_amd
        from rtw_amd import _capi
        self.torch, self.rtw, self.L, self.T, self.S = torch, rtw_amd, _capi.lib(), T, S
        self.W, self.H = size
        self.n = self.W * self.H
        self.inputs = _inputs(size, T)[:S]
        self.n_state, self.n_mom = TR.state_elems(self.H, self.W, T), NR.moment_elems(self.H, self.W, T)
        eb = np.dtype(T).itemsize
        assert self.n_state * eb == self.L.rtw_temporal_state_bytes(self.W, self.H, eb) and self.n_mom * eb == self.L.rtw_history_moment_bytes(self.W, self.H, eb)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        self.host = [(PR.pack_frames([i[1][k][0] for i in self.inputs]), PR.pack_frames([i[1][k][1] for i in self.inputs])) for k in range(3)]
        self.dev = [(up(i), up(f)) for i, f in self.host]
        self.host0 = (PR.pack_states([i[2] for i in self.inputs], T), PR.pack_moments([i[3] for i in self.inputs], T))
        self.state0, self.moment0 = up(self.host0[0]), up(self.host0[1])
        self.cam0 = [i[4] for i in self.inputs]
        torch.cuda.synchronize()

    def cams(self, k):
        return [i[0][k] for i in self.inputs]

    def table(self, k, cams_prev):
        """the uploaded table of step k (cams_prev None: first frames), one spare entry of -7 behind it"""
        tab = np.full((self.S + 1, 32), -7.0, self.T)
        tab[:self.S] = self.rtw.temporal_path_table(self.cams(k), cams_prev, self.T)
        return self.torch.from_numpy(tab.reshape(-1)).to("cuda:0")

    def buffers(self, poison=-7.0):
        """-> (next states, next moment planes, out + one spare frame), filled with `poison`"""
        dt = self.dev[0][0].dtype
        return tuple(self.torch.full((k,), poison, dtype=dt, device="cuda:0") for k in (self.S * self.n_state, self.S * self.n_mom, (self.S + 1) * self.n * 3))

    def batch(self, k, table, form, states=None, moments_prev=None, bufs=None, images=None, feats=None, **kw):
        """rtw_reproject_batch_device_* on frame k of every path -> bufs, synchronised"""
        from rtw_amd import _capi
        moments, clamp = FORMS[form]
        bufs = self.buffers() if bufs is None else bufs
        self.torch.cuda.synchronize()                              # the fills ran on torch's stream
        img, feat = self.dev[k]
        img, feat = (img if images is None else images), (feat if feats is None else feats)
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _capi.check(getattr(self.L, "rtw_reproject_batch_device_" + _sfx(self.T))(
            C.byref(_tparams(**dict(STEP_KW, **kw))), C.byref(_cparams(**clamp)) if clamp else None, self.S, vp(table), self.W, self.H, vp(img), vp(feat), vp(states),
            vp(moments_prev) if moments and states is not None else None, vp(bufs[0]), vp(bufs[1]) if moments else None, vp(bufs[2]), None))
        self.torch.cuda.synchronize()
        return bufs

    def single(self, s, k, form, cam_prev, states=None, moments_prev=None, **kw):
        """the single device call of the form on path s's slices of the same tensors -> (next state, next moment plane, out) of ONE path"""
        from rtw_amd import _capi
        moments, clamp = FORMS[form]
        dt = self.dev[0][0].dtype
        nxt, mom, out = (self.torch.full((n,), -7.0, dtype=dt, device="cuda:0") for n in (self.n_state, self.n_mom, self.n * 3))
        self.torch.cuda.synchronize()
        img, feat = self.dev[k][0][s * self.n * 3:], self.dev[k][1][s * self.n * 8:]
        sp = states[s * self.n_state:] if states is not None else None
        mp = moments_prev[s * self.n_mom:] if moments and states is not None else None
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        Cm = _capi.make_camera(self.cams(k)[s], self.T)
        Cp = C.byref(_capi.make_camera(cam_prev, self.T)) if cam_prev is not None else None
        t = C.byref(_tparams(**dict(STEP_KW, **kw)))
        if clamp:
            rc = getattr(self.L, "rtw_clamped_step_device_" + _sfx(self.T))(t, C.byref(_cparams(**clamp)), C.byref(Cm), Cp, self.W, self.H, vp(img), vp(feat), vp(sp), vp(mp), vp(nxt),
                                                                              vp(mom) if moments else None, vp(out), None)
        elif moments:
            rc = getattr(self.L, "rtw_history_moments_device_" + _sfx(self.T))(t, C.byref(Cm), Cp, self.W, self.H, vp(img), vp(feat), vp(sp), vp(mp), vp(nxt), vp(mom), vp(out), None)
        else:
            rc = getattr(self.L, "rtw_temporal_device_" + _sfx(self.T))(t, C.byref(Cm), Cp, self.W, self.H, vp(img), vp(feat), vp(sp), vp(nxt), vp(out), None)
        _capi.check(rc)
        self.torch.cuda.synchronize()
        return nxt, mom, out

    def result(self, bufs, moments):
        """-> per path (out, state, moment plane or None) in the witnesses' layout"""
        st, mo, out = (b.cpu().numpy() for b in bufs)
        outs = PR.unpack_frames(out[:self.S * self.n * 3], self.S, self.H, self.W, 3)
        sts = PR.unpack_states(st, self.S, self.H, self.W)
        mos = PR.unpack_moments(mo, self.S, self.H, self.W) if moments else [None] * self.S
        return list(zip(outs, sts, mos))

    def inputs_unchanged(self):
        same = lambda t, a: np.array_equal(DR.bits(t.cpu().numpy()), DR.bits(a))
        return all(same(d[0], h[0]) and same(d[1], h[1]) for d, h in zip(self.dev, self.host)) and same(self.state0, self.host0[0]) and same(self.moment0, self.host0[1])


def _assert_step(got, ref, what):
    _assert_same(got[0], ref[0], what + ": image")
    for k in ("E", "G", "L"):
        _assert_same(got[1][k], ref[1][k], f"{what}: state plane {k}")
    assert (got[2] is None) == (ref[2] is None), what
    if ref[2] is not None:
        _assert_same(got[2], ref[2], what + ": moment plane")


def _bits(t):
    return DR.bits(t.cpu().numpy())


# ---- 1. the batched device step equals the witness and the single device call of every path ----------------------------------------------------
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("T", TYPES)
def test_the_batched_step_equals_the_witness_and_the_single_calls(T, size, S):
    dev = PathFrames(size, T, S)
    n, ns, nm = dev.n, dev.n_state, dev.n_mom
    for form, (moments, _) in FORMS.items():
        for start in ("first", "state"):
            ref = _chain(size, T, form, start)
            states, mprev, cams_prev = (None, None, None) if start == "first" else (dev.state0, dev.moment0, dev.cam0)
            for k in range(3):
                what = f"{np.dtype(T).name} {size} S={S} {form} from {start}, step {k}"
                bufs = dev.batch(k, dev.table(k, cams_prev), form, states, mprev)
                got = dev.result(bufs, moments)
                for s in range(S):
                    _assert_step(got[s], ref[k][s], f"{what}, path {s}")
                    one = dev.single(s, k, form, cams_prev[s] if cams_prev else None, states, mprev)
                    assert np.array_equal(_bits(one[0][:9 * n]), _bits(bufs[0][s * ns:s * ns + 9 * n])), f"{what}, path {s}: state vs the single call"
                    assert np.array_equal(_bits(one[2]), _bits(bufs[2][s * n * 3:(s + 1) * n * 3])), f"{what}, path {s}: image vs the single call"
                    if moments:
                        assert np.array_equal(_bits(one[1][:n]), _bits(bufs[1][s * nm:s * nm + n])), f"{what}, path {s}: moment plane vs the single call"
                states, mprev, cams_prev = bufs[0], bufs[1], dev.cams(k)
    assert dev.inputs_unchanged()


# ---- 2. isolation: what the other paths hold decides nothing ----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["moments", "clamped+guides+moments"])
@pytest.mark.parametrize("T", TYPES)
def test_a_path_does_not_see_its_neighbours(T, form):
    import torch
    size, S = (37, 23), 3
    dev = PathFrames(size, T, S)
    n, ns, nm = dev.n, dev.n_state, dev.n_mom
    table = dev.table(0, dev.cam0)
    base = [b.clone() for b in dev.batch(0, table, form, dev.state0, dev.moment0)]
    for s in range(S):
        for poison in (float("nan"), 1e30):
            img, feat, st, mo = dev.dev[0][0].clone(), dev.dev[0][1].clone(), dev.state0.clone(), dev.moment0.clone()
            keep = (img[s * n * 3:(s + 1) * n * 3].clone(), feat[s * n * 8:(s + 1) * n * 8].clone(), st[s * ns:(s + 1) * ns].clone(), mo[s * nm:(s + 1) * nm].clone())
            for t, own, width in ((img, keep[0], n * 3), (feat, keep[1], n * 8), (st, keep[2], ns), (mo, keep[3], nm)):
                t.fill_(poison)
                t[s * width:(s + 1) * width] = own
            torch.cuda.synchronize()
            bufs = dev.batch(0, table, form, st, mo, images=img, feats=feat)
            what = f"{np.dtype(T).name} {form}: path {s} with its neighbours replaced by {poison}"
            assert np.array_equal(_bits(bufs[0][s * ns:(s + 1) * ns]), _bits(base[0][s * ns:(s + 1) * ns])), what + ": state"
            assert np.array_equal(_bits(bufs[1][s * nm:(s + 1) * nm]), _bits(base[1][s * nm:(s + 1) * nm])), what + ": moment plane"
            assert np.array_equal(_bits(bufs[2][s * n * 3:(s + 1) * n * 3]), _bits(base[2][s * n * 3:(s + 1) * n * 3])), what + ": image"


# ---- 3. poisoned outputs change nothing; padding and what lies behind the last path are never written -------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (37, 23)])
@pytest.mark.parametrize("T", TYPES)
def test_poisoned_outputs_change_nothing_and_the_padding_is_kept(T, size):
    S = 3
    dev = PathFrames(size, T, S)
    n, ns, nm = dev.n, dev.n_state, dev.n_mom
    assert ns > 9 * n and nm > n                                  # (W*H is odd: there IS padding)
    table = dev.table(0, dev.cam0)
    for form in ("moments", "clamped+moments"):
        ref = _chain(size, T, form, "state")[0]
        for poison in (float("nan"), float("inf"), 1e30):
            bufs = dev.batch(0, table, form, dev.state0, dev.moment0, bufs=dev.buffers(poison))
            for s, got in enumerate(dev.result(bufs, True)):
                _assert_step(got, ref[s], f"{np.dtype(T).name} {size} {form} poison {poison}, path {s}")
            st, mo, out = (b.cpu().numpy() for b in bufs)
            assert np.array_equal(DR.bits(PR.state_padding(st, S, dev.H, dev.W)), DR.bits(np.full((S, ns - 9 * n), poison, T)))
            assert np.array_equal(DR.bits(PR.moment_padding(mo, S, dev.H, dev.W)), DR.bits(np.full((S, nm - n), poison, T)))
            assert np.array_equal(DR.bits(out[S * n * 3:]), DR.bits(np.full(n * 3, poison, T)))
    # without moments the moment buffer is not the kernel's to write; a first frame reads no state
    for form in ("plain", "clamped"):
        bufs = dev.batch(0, table, form, dev.state0, dev.moment0, bufs=dev.buffers(1e30))
        assert np.array_equal(_bits(bufs[1]), DR.bits(np.full(S * nm, 1e30, T)))
    assert dev.inputs_unchanged()


# ---- 4. every table element reaches the kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "clamped+moments"])
@pytest.mark.parametrize("T", TYPES)
def test_every_table_element_reaches_the_kernel(T, form):
    size, S, s = (37, 23), 3, 1
    dev = PathFrames(size, T, S)
    n, ns = dev.n, dev.n_state
    table = dev.table(0, dev.cam0)
    base = [b.clone() for b in dev.batch(0, table, form, dev.state0, dev.moment0)]
    host = table.cpu().numpy().copy()
    for e in range(32):
        tab = host.copy()
        tab[s * 32 + e] = tab[s * 32 + e] * T(1.125) + T(0.0625)
        bufs = dev.batch(0, dev.torch.from_numpy(tab).to("cuda:0"), form, dev.state0, dev.moment0)
        same = [np.array_equal(_bits(bufs[0][p * ns:(p + 1) * ns]), _bits(base[0][p * ns:(p + 1) * ns])) and
                np.array_equal(_bits(bufs[2][p * n * 3:(p + 1) * n * 3]), _bits(base[2][p * n * 3:(p + 1) * n * 3])) for p in range(S)]
        assert same[0] and same[2], f"{form}: element {e} of path {s} changed another path"
        assert same[s] == (e >= 29), f"{form}: element {e} of path {s}: {'read' if e >= 29 else 'not read'}"
    # the spare entry behind the table is not read, and a first frame reads no entry at all
    tab = host.copy()
    tab[S * 32:] = np.nan
    bufs = dev.batch(0, dev.torch.from_numpy(tab).to("cuda:0"), form, dev.state0, dev.moment0)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(bufs, base))
    first = [b.clone() for b in dev.batch(0, table, form)]
    bufs = dev.batch(0, dev.torch.full_like(table, float("nan")), form)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(bufs, first))


# ---- 5. the batched noise map equals the single one of every path ------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (37, 23), (70, 40)])
@pytest.mark.parametrize("T", TYPES)
def test_the_batched_noise_map_equals_the_single_maps(T, size, S):
    import torch
    from rtw_amd import _capi
    dev = PathFrames(size, T, S)
    n, ns, nm = dev.n, dev.n_state, dev.n_mom
    ref = _chain(size, T, "moments", "state")[0]
    bufs = dev.batch(0, dev.table(0, dev.cam0), "moments", dev.state0, dev.moment0)
    vp = lambda t: C.c_void_p(t.data_ptr())
    for nk in (dict(NR.NOISE_DEFAULTS), dict(radius=1, m=0, min_len=1.0), dict(radius=3, m=1, min_len=8.0)):
        rho = torch.full(((S + 1) * n,), -7.0, dtype=bufs[0].dtype, device="cuda:0")
        torch.cuda.synchronize()
        _capi.check(getattr(dev.L, "rtw_reproject_noise_batch_device_" + _sfx(T))(C.byref(_nparams(**nk)), dev.W, dev.H, S, vp(bufs[0]), vp(bufs[1]), vp(rho), None))
        torch.cuda.synchronize()
        assert (rho[S * n:] == -7.0).all()
        for s, got in enumerate(PR.unpack_frames(rho[:S * n].cpu().numpy(), S, dev.H, dev.W)):
            what = f"{np.dtype(T).name} {size} S={S} {nk}, path {s}"
            _assert_same(got, NR.noise_map(ref[s][1], ref[s][2], T, **nk), what + ": the witness")
            one = torch.full((n,), -7.0, dtype=bufs[0].dtype, device="cuda:0")
            torch.cuda.synchronize()
            _capi.check(getattr(dev.L, "rtw_history_noise_device_" + _sfx(T))(C.byref(_nparams(**nk)), dev.W, dev.H, vp(bufs[0][s * ns:]), vp(bufs[1][s * nm:]), vp(one), None))
            torch.cuda.synchronize()
            assert np.array_equal(_bits(one), _bits(rho[s * n:(s + 1) * n])), what + ": the single call"


# ---- 6. the paths call equals the sequence calls, path by path ----------------------------------------------------------------------------------
def _paths(rtw, T, S, N):
    return [[rtw.default_camera(lookfrom=(1.5 * np.sin(0.25 * k) + 0.07 * s, 0.4 + 0.05 * s, -1 + 1.5 * np.cos(0.25 * k)), lookat=(0.03 * s, 0, -1), vfov=60, aperture=0, elem_type=T)
             for k in range(N)] for s in range(S)]


@pytest.mark.parametrize("T", TYPES)
def test_render_paths_equals_the_sequence_calls(rtw, T):
    """S = 3 paths of N = 3 steps at 48x27, 1 spp, over the two-sphere scene, in all four forms (no filter, the plain filter, guided, and
    clamped with each of the three): path s against rtw_render_sequence_* / _path_guided_* / _path_clamped_* of its own cameras and seeds, on
    the bits; rtw_stats reports the batched render's record"""
    W, H, S, N = 48, 27, 3, 3
    scene, paths = rtw.scene_2_spheres(elem_type=T), _paths(rtw, T, S, N)
    seeds = [[100 * s + k + 1 for k in range(N)] for s in range(S)]
    tkw = dict(normal_power_log2=1, sigma_depth=0.2, min_weight=0.125, history_max=6.0)
    nkw = dict(radius=2, normal_power_log2=1, sigma_depth=0.1, min_len=2.0)
    dkw = dict(levels=2, sigma_color=1.5)
    ck = dict(radius=2, guides=True, sigma=1.0, len_scale=0.5)
    rtw.render_batch(scene, [paths[s][k] for k in range(N) for s in range(S)], W, 1, seed=[seeds[s][k] for k in range(N) for s in range(S)], gamma=False)
    batch_stats = {k: rtw.last_stats()[k] for k in _STAT_KEYS}
    distinct = set()
    for clamp in (None, ck):
        for form in ("none", "plain", "guided"):
            kw = dict(clamp=clamp, gamma=form != "plain", denoise=None if form == "none" else dkw, guided=nkw if form == "guided" else None, **tkw)
            got = rtw.render_sequences(scene, paths, W, 1, seeds=seeds, **kw)
            assert got.shape == (S, N, H, W, 3) and got.dtype == T and np.isfinite(got).all()
            assert {k: rtw.last_stats()[k] for k in _STAT_KEYS} == batch_stats
            for s in range(S):
                ref = rtw.render_sequence(scene, paths[s], W, 1, seeds=seeds[s], **kw)
                for k in range(N):
                    _assert_same(got[s, k], ref[k], f"{np.dtype(T).name} clamp={clamp is not None} {form}: path {s}, step {k}")
            distinct.add(DR.bits(np.ascontiguousarray(got)).tobytes())
    assert len(distinct) == 6                                       # (the six forms are six different results)
    # one path of one step, and one path alone, through the same call
    one = rtw.render_sequences(scene, [paths[1]], W, 1, seeds=[seeds[1]], clamp=ck, **tkw)
    _assert_same(one[0], rtw.render_sequence(scene, paths[1], W, 1, seeds=seeds[1], clamp=ck, **tkw), "a single path")


# ---- 7. the Python layer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "clamped+guides+moments"])
def test_the_batch_accumulator_equals_the_chain(rtw, form):
    import torch
    T, size, S = np.float32, (37, 23), 3
    W, H = size
    dev = PathFrames(size, T, S)
    moments, clamp = FORMS[form]
    ref = _chain(size, T, form, "first")
    acc = rtw.TemporalBatchAccumulator(S, W, H, elem_type=T, moments=moments, clamp=clamp, normal_power_log2=STEP_KW["m"])
    out = torch.zeros(S * W * H * 3, dtype=torch.float32, device="cuda:0")
    rho = torch.zeros(S * W * H, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert acc.state(0) is None
    for k in range(3):
        acc.step(dev.cams(k), dev.dev[k][0].data_ptr(), dev.dev[k][1].data_ptr(), out.data_ptr())
        if moments:
            acc.noise_into(rho.data_ptr())
        torch.cuda.synchronize()
        outs = PR.unpack_frames(out.cpu().numpy(), S, H, W, 3)
        for s in range(S):
            got = (outs[s], TR.unpack_state(acc.state(s).cpu().numpy(), H, W), NR.unpack_moment(acc.moment(s).cpu().numpy(), H, W) if moments else None)
            _assert_step(got, ref[k][s], f"TemporalBatchAccumulator {form}, step {k}, path {s}")
            if moments:
                _assert_same(PR.unpack_frames(rho.cpu().numpy(), S, H, W)[s], NR.noise_map(ref[k][s][1], ref[k][s][2], T), f"noise_into, step {k}, path {s}")
    assert acc.frames == 3
    acc.reset()
    assert acc.state(1) is None and acc.frames == 0
    acc.step(dev.cams(0), dev.dev[0][0].data_ptr(), dev.dev[0][1].data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    _assert_same(PR.unpack_frames(out.cpu().numpy(), S, H, W, 3)[2], ref[0][2][0], "after reset: a first frame again")
    with pytest.raises(ValueError):
        acc.step(dev.cams(0)[:2], dev.dev[0][0].data_ptr(), dev.dev[0][1].data_ptr(), out.data_ptr())
    if not moments:
        with pytest.raises(ValueError):
            acc.noise_into(rho.data_ptr())
