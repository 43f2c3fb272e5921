"""The block vote of the group cull on the matrix pipe (hit_world_mfma<.., CULLED>, `block_sets`), ray by ray against exact box overlap.

Unit op 27 is op 20's scan with a sink that also records the vote; op 28 returns the cull layout.  Slots per ray (8 bytes each):
  op 27  in  o[3] d[3] tmin tmax      out ok, mf_sc, candidate bits [8 x uint64], in-lane bits [8 x uint64] (bit i = sphere i, as ops 17 - 20),
                                           voted blocks (raw uint64: bit b = block b of the device order was voted for by this ray's half wave)
  op 28  in  (one slot, ignored)      out item p = device position p (block p / 32): the caller's index of the sphere there or -1 (dead, padding,
                                           beyond the layout), 1 if the position is in the in-lane list, the number of positions, of blocks

The 32 rays of a half wave OR their sets, so a block one ray wrongly drops is normally voted in by its neighbours.  Here a wave holds the ray
under test in chosen lanes and a far-miss ray -- above the class box, pointing away: its own set is the infinite boxes only -- in all others:
  lanes   the ray in exactly one lane, for each of tests/vote_cases.LANES (every 16-lane row, both halves, both ends of the DPP butterflies)
  rows    the ray in one 16-lane row
  halves  the ray in all 32 lanes of a half
  short   launches of 1, 17 and 33 rays: lanes with no ray at all
Per wave: the tested half's word holds must(ray) and lies inside may(ray) (tests/exact_vote.py: exact box overlap, and the allowance the
design grants); the other half's word IS the far-miss set; op 20's rule (candidates + in-lane >= the oracle's hits) and op 14's answer (== the
oracle's hit_world, bit for bit) hold on the same waves.  tests/test_exact_vote.py checks on the CPU that the rays make these bite."""
import numpy as np
import pytest

import exact_vote as V
import vote_cases as VC
from test_gpu_filters import oracle_sets
from test_gpu_units import run_unit

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("numerics")]
F = [np.float32, np.float64]
KINDS = {"lanes": [f"lane{l}" for l in VC.LANES], "rows": [f"row{q}" for q in range(4)], "halves": ["half0", "half1"]}


def tmin_of(T):
    return float(T(1e-3))


_LAYOUT = {}


def device_case(name, T):
    """the scene judged with the DEVICE's layout (op 28) -- which must be the recorded one the CPU test judged"""
    if (name, T) not in _LAYOUT:
        flat = VC.scenes(T)[name]
        lay = V.layout_of(run_unit(28, np.zeros((VC.MAX_POSITIONS, 1)), 4, T, flat=flat))
        rec = VC.recorded_layout(name, T)
        assert lay.n_blocks == rec.n_blocks and np.array_equal(lay.idx, rec.idx) and np.array_equal(lay.inlane, rec.inlane), \
            (name, "the cull layout differs from tests/golden/cull_layouts.npz: record it again (op 28) and rerun tests/test_exact_vote.py")
        _LAYOUT[(name, T)] = True
    return VC.judged(name, T)


def run_vote(flat, x, T):
    """op 27 -> ok [m], vote word [m] (uint64), the raw rows"""
    y = run_unit(27, x, 19, T, flat=flat)
    return y[:, 0] != 0, np.ascontiguousarray(y[:, 18]).view(np.uint64), y


def bits_of(rows):
    return np.unpackbits(np.ascontiguousarray(rows).view(np.uint64).astype("<u8").view(np.uint8), bitorder="little").reshape(len(rows), 512).astype(bool)


_ORACLE = {}


def oracle_case(oracle, key, flat, o, d, T):
    """(idx, t, hit set [m, n]) of the unique rays (the last one: the far-miss ray), once per scene, precision and numerics mode"""
    if key not in _ORACLE:
        with np.errstate(invalid="ignore", over="ignore"):
            idx, t = oracle.hit_world_batch(flat, np.concatenate([o, d], 1).astype(T), T(tmin_of(T)), np.inf, T)
            _, _, hset = oracle_sets(oracle, flat, o, d, tmin_of(T), np.full(len(o), np.inf), T)
        _ORACLE[key] = (idx.astype(np.int64), t.astype(np.float64), hset)
    return _ORACLE[key]


def words_of(M, sets):
    return np.array([M.word(s) if s is not None else 0 for s in sets], np.uint64)


def check_waves(oracle, numerics, name, T, placement, lanes, case, sel=None, count=None):
    """one launch of op 27 and one of op 14: a wave per ray of `sel` with the ray in `lanes`; count: the launch's length (a short last wave)"""
    flat, M, fam, o, d, ok, must, may, fo, fd = case
    sel = np.arange(len(o)) if sel is None else np.asarray(sel)
    m, n = len(sel), flat["n"]
    finite = np.array([must[j] is not None for j in sel])
    x = VC.waves(o[sel], d[sel], fo, fd, lanes, tmin_of(T))
    if count is not None:
        x = x[:count]
    live = np.zeros(m * 64, bool); live[:len(x)] = True
    live = live.reshape(m, 64)
    tested = np.zeros((m, 64), bool); tested[:, lanes] = True
    tested &= live
    okd, w, y = run_vote(flat, x, T)
    pad = lambda a, fill: np.concatenate([a, np.full(m * 64 - len(a), fill, a.dtype)]).reshape(m, 64)
    okd, w = pad(okd, False), pad(w, np.uint64(0))
    tag = (name, VC.tname(T), numerics, placement)
    # the range answer, every ray (the non-finite ones too)
    want_ok = np.where(tested, ok[sel][:, None], True)
    assert np.array_equal(okd[live], want_ok[live]), (tag, "ok", np.argwhere(live & (okd != want_ok))[:5])
    # one word per half
    h = lanes[0] // 32
    assert all(l // 32 == h for l in lanes)
    for hh in (0, 1):
        half = slice(32 * hh, 32 * hh + 32)
        first = w[:, 32 * hh][:, None]
        assert (~live[:, half] | (w[:, half] == first)).all(), (tag, "the lanes of a half wave report different words")
    far_w = np.uint64(M.word(M.big))
    live_o = live[:, 32 * (1 - h)]
    assert (w[live_o, 32 * (1 - h)] == far_w).all(), (tag, "the far-miss half", [hex(int(v)) for v in np.unique(w[live_o, 32 * (1 - h)])], hex(int(far_w)))
    got = w[:, 32 * h]
    mustw, mayw = words_of(M, [must[j] for j in sel]), words_of(M, [may[j] for j in sel])
    lost = finite & ((got & mustw) != mustw)
    assert not lost.any(), (tag, "a block the ray meets was not voted for", [(int(sel[i]), VC.FAMILIES[fam[sel[i]]], hex(int(got[i])), hex(int(mustw[i])), o[sel[i]].tolist(), d[sel[i]].tolist()) for i in np.flatnonzero(lost)[:4]])
    wide = finite & ((got & ~mayw) != 0)
    assert not wide.any(), (tag, "a vote beyond the allowance", [(int(sel[i]), VC.FAMILIES[fam[sel[i]]], hex(int(got[i])), hex(int(mayw[i])), o[sel[i]].tolist(), d[sel[i]].tolist()) for i in np.flatnonzero(wide)[:4]])
    # op 20's rule on the same waves: the tested lanes' rows and one far-miss row per wave
    uo, ud = np.concatenate([o, fo[None]]), np.concatenate([d, fd[None]])
    ref_idx, ref_t, hset = oracle_case(oracle, (name, T, numerics), flat, uo, ud, T)
    rows = y.reshape(-1, 19)
    lane0 = lanes[0]
    pick = np.flatnonzero(finite & live[:, lane0])
    have = bits_of(rows[pick * 64 + lane0, 2:10]) | bits_of(rows[pick * 64 + lane0, 10:18])
    miss = hset[sel[pick]] & ~have[:, :n]
    assert not miss.any(), (tag, "candidates + in-lane < the oracle's hits", np.argwhere(miss)[:5])
    far_lane = next(l for l in range(64) if l not in lanes)
    pick = np.flatnonzero(live[:, far_lane])
    have = bits_of(rows[pick * 64 + far_lane, 2:10]) | bits_of(rows[pick * 64 + far_lane, 10:18])
    assert have[:, :n][:, hset[-1]].all(), (tag, "a far-miss lane lost a candidate")
    # op 14 on the same waves == the oracle's closest hit (the waves of a non-finite ray: the other lanes only)
    y14 = run_unit(14, x, 9, T, flat=flat)
    which = np.where(tested, sel[:, None], len(o)).reshape(-1)[:len(x)]
    judge = (live & (~tested | finite[:, None])).reshape(-1)[:len(x)]
    bad = judge & ((y14[:, 0].astype(np.int64) != ref_idx[which]) | ((ref_idx[which] >= 0) & (y14[:, 1] != ref_t[which])))
    assert not bad.any(), (tag, "op 14", int(bad.sum()), np.flatnonzero(bad)[:5], y14[bad][:3, :2], ref_idx[which][bad][:3])
    return got, finite


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("T", F)
@pytest.mark.parametrize("name", VC.SCENES)
def test_vote_of_one_ray_among_far_misses(oracle, numerics, name, T, kind):
    case = device_case(name, T)
    flat, M, fam, o, d, ok, must, may, fo, fd = case
    # the far-miss ray by itself: the infinite boxes only (a wave of nothing else)
    okd, w, _ = run_vote(flat, VC.waves(fo[None], fd[None], fo, fd, [0], tmin_of(T)), T)
    assert okd.all() and (w == np.uint64(M.word(M.big))).all(), (name, [hex(int(v)) for v in np.unique(w)])
    P = VC.placements()
    for placement in KINDS[kind]:
        got, finite = check_waves(oracle, numerics, name, T, placement, P[placement], case)
        if placement == "half0" and M.finite:
            # ungated: the ray's own set against exact overlap -- the share of voted (ray, block) pairs beyond must, and how far outside
            # the ungrown overlap the farthest voted block lay, as a fraction of the allowance
            fin_w = np.uint64(M.word(M.finite))
            voted = extra = 0
            worst = 0.0
            for j in np.flatnonzero(finite & ok):
                v = int(got[j] & fin_w)
                beyond = frozenset(b for b in M.finite if v >> b & 1) - must[j]
                voted += bin(v).count("1"); extra += len(beyond)
                if beyond:
                    worst = max(worst, M.may(VC.as_kernel(o[j]), VC.as_kernel(d[j]), excess_of=beyond)[1])
            print(f"vote record {name} {VC.tname(T)}: {voted} voted pairs, {extra} beyond must ({100.0 * extra / max(voted, 1):.1f} %), largest excess {worst:.3f} A")


@pytest.mark.parametrize("T", F)
@pytest.mark.parametrize("name", VC.SCENES)
def test_vote_of_short_waves(oracle, numerics, name, T):
    """launches of 1, 17 and 33 rays: the ray under test in the last lane, far-miss rays in front of it, NO ray behind it.  With 1 and 33
    rays the tested half holds nothing else: its word is the ray's own set."""
    case = device_case(name, T)
    flat, M, fam, o, d, ok, must, may, fo, fd = case
    fin = [j for j in range(len(o)) if must[j] is not None]
    j1 = next((j for j in fin if ok[j] and must[j] - M.big and may[j] != M.live), fin[0])
    j2 = next(j for j in fin if not ok[j])
    for count in (1, 17, 33):
        for j in (j1, j2):
            check_waves(oracle, numerics, name, T, f"short{count}", [count - 1], case, sel=[j], count=count)


def _plain_rays(flat, rng, T):
    """rays for a scene without a layout at hand: nearly axis-aligned ones through the class, rays from sphere surfaces, rays along and
    across the layer, rays pointing away"""
    c = np.stack([flat["cx"], flat["cy"], flat["cz"]], 1).astype(np.float64)
    r = np.abs(flat["r"].astype(np.float64))
    lo, hi = (c - r[:, None]).min(0), (c + r[:, None]).max(0)
    size = float((hi - lo).max())
    o, d = [], []
    for a in range(3):
        for sg in (1.0, -1.0):
            for k in range(10):
                p = lo + rng.uniform(0, 1, 3) * (hi - lo)
                if k % 3 == 1:
                    p[a] = (lo[a] - 0.2 * size) if sg > 0 else (hi[a] + 0.2 * size)
                if k % 3 == 2:
                    p[a] = float(T(lo[a] if k % 2 else hi[a]))
                dd = np.zeros(3)
                dd[a] = sg
                dd[(a + 1) % 3] = VC.SMALL[int(rng.integers(len(VC.SMALL)))]
                dd[(a + 2) % 3] = VC.SMALL[int(rng.integers(len(VC.SMALL)))]
                o.append(p); d.append(dd)
    for i in rng.choice(len(r), 30, replace=False):
        nrm = VC._unit(rng.normal(size=3))
        for dd in (nrm, -nrm, VC._unit(np.cross(nrm, rng.normal(size=3)))):
            o.append(c[i] + r[i] * nrm); d.append(dd)
    for a in range(3):
        for sg in (1.0, -1.0):
            p = lo + rng.uniform(0, 1, 3) * (hi - lo)
            p[a] = (hi[a] if sg > 0 else lo[a]) + sg * 0.1 * size
            dd = rng.normal(size=3) * 0.5
            dd[a] = sg * (0.6 + abs(dd[a]))
            o.append(p); d.append(VC._unit(dd))
    far_o = (lo + hi) / 2
    far_o[1] = hi[1] + size
    return np.array(o).astype(T).astype(np.float64), np.array(d).astype(T).astype(np.float64), far_o.astype(T).astype(np.float64), np.array([0.0, 1.0, 0.0])


@pytest.mark.parametrize("T", F)
def test_two_groups_of_tables_through_op_14(oracle, numerics, T):
    """1 100 spheres: two groups of 32 blocks, each with tables of its own -- beyond the sinks (RTW_SINK_SPHERES).  The same placements through
    op 14 alone: a block one ray needs and its far-miss neighbours do not must still be visited, in either group."""
    from test_gpu_round5 import _vote_scenes
    flat = _vote_scenes(T)["two_groups_lds"]
    o, d, fo, fd = _plain_rays(flat, np.random.default_rng(41), T)
    rays = np.concatenate([np.concatenate([o, fo[None]]), np.concatenate([d, fd[None]])], 1)
    ref_idx, ref_t = oracle.hit_world_batch(flat, rays.astype(T), T(tmin_of(T)), np.inf, T)
    assert ref_idx[-1] < 0 and (ref_idx[:-1] >= 0).sum() >= 60 and len({int(i) // 32 for i in ref_idx if i >= 0}) >= 16
    xs, which = [], []
    for placement, lanes in VC.placements().items():
        xs.append(VC.waves(o, d, fo, fd, lanes, tmin_of(T)))
        w = np.full((len(o), 64), len(o)); w[:, lanes] = np.arange(len(o))[:, None]
        which.append(w.reshape(-1))
    x, which = np.concatenate(xs), np.concatenate(which)
    y = run_unit(14, x, 9, T, flat=flat)
    bad = (y[:, 0].astype(np.int64) != ref_idx[which]) | ((ref_idx[which] >= 0) & (y[:, 1] != ref_t.astype(np.float64)[which]))
    assert not bad.any(), (numerics, int(bad.sum()), np.flatnonzero(bad)[:5], y[bad][:3, :2], ref_idx[which][bad][:3])
