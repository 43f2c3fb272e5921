"""The two-stage evaluation of the matrix-pipe filter (csrc/rtw_scan_mfma.hpp, "Two stages"): per ray half and block the plain scan issues the
first MFMA of the pair, and the second only where some lane's coarse value is not negative.  One wave of hand-made rays per case against a
scene of 32 + 32 + 6 spheres, unit ops 13 / 14 (closest hit) and their candidate sinks 19 / 20, both precisions, every numerics mode.

Scene: 70 spheres of radius 0.5 in three clusters 100 apart along x, centres on a dyadic grid (exact in binary32, r^2 exact), in the caller's
order = the block order of op 13 (the kd split of op 14 cuts x at the same places).  Rays run along +z from z = -50 ("near") or from 0.9 x the
filter's |o| limit ("far", where the coarse margin is largest); the lanes of one ray half aim at one block, the other half passes far above
everything.  What the lanes of the aimed half do per kind:
    hit     through a column of the block, 0.2 beside the centres            the fine test finds candidates (and the ray hits)
    d0      0.5 beside: D = 0 exactly for the aimed sphere                    a candidate by the superset rule
    edge    D = -0.99 x the band of tests/exact_filters.py                    a candidate by the band rule
    coarse  1.3 (near) / 60 (far) beside the column in y                      the coarse test leaves the half open, the fine test finds nothing
    (the other half, and the waves of kind `none`)                            the coarse test settles the half
Which of the three paths a (ray half, block) cell takes is decided by the EXACT coarse and fine values of its 32 x 32 pairs
(tests/two_stage_check.cpp --pairs: the host's operands x a host mirror of the prologue's, in integer arithmetic) against the error bounds of
the two MFMAs -- asserted for the aimed cell of every case, so each case is what it claims to be -- and wherever the exact fine value is
decisive the device's candidate bit must agree with its sign: a pair is a candidate if W > E1 + E2 and none if W < -(E1 + E2), whichever
path its half took.  Asserted besides: index and t_hit of every lane equal the oracle's closest hit bit for bit; candidates cover the
oracle's set (op 14: its hits) and the band.  Every case also runs with 20 / 40 / 48 lanes that have a ray and with one ray off the filter."""
import os
import subprocess

import numpy as np
import pytest

import exact_filters as X
from test_gpu_filters import centres, exact_classes, make_flat, oracle_sets, run_sink
from test_gpu_units import run_unit

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("numerics")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, BLOCKS, R = 70, [range(0, 32), range(32, 64), range(64, 70)], 0.5
TMIN = 1e-3
KINDS = ("hit", "d0", "edge", "coarse")


def scene(T):
    c = np.zeros((N, 3))
    for b, blk in enumerate(BLOCKS):
        for j, i in enumerate(blk):
            c[i] = [100.0 * (b - 1) + j / 64.0, 3.0 * (j % 8), 3.0 * (j // 8)]
    return make_flat(c, np.full(N, R), T)


_TOOL = {}


def model(flat, o, d, tmp):
    """exact (P1', E1, W, E2) [m, N] of every pair and ok [m], from the CPU check program (kept per set of rays: the numerics modes share it)"""
    key = (o.tobytes(), d.tobytes())
    if key in _TOOL:
        return _TOOL[key]
    if "exe" not in _TOOL:
        exe = os.path.join(str(tmp), "two_stage_check")
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "two_stage_check.cpp")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        _TOOL["exe"] = exe
    c, r = centres(flat)
    path = os.path.join(str(tmp), "pairs.txt")
    with open(path, "w") as f:
        f.write(f"{N}\n")
        for i in range(N):
            f.write(" ".join(float(v).hex() for v in (*c[i], r[i])) + "\n")
        f.write(f"{len(o)}\n")
        for i in range(len(o)):
            f.write(" ".join(float(v).hex() for v in (*o[i], *d[i])) + " 1\n")
    out = subprocess.run([_TOOL["exe"], "--pairs", path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-500:]
    ok, vals = [], []
    for line in out.stdout.splitlines():
        if line.startswith("ray"):
            ok.append(line.split()[1] == "1")
        else:
            vals.append([float.fromhex(v) for v in line.split()])
    v = np.array(vals).reshape(len(o), N, 4)
    _TOOL[key] = (np.array(ok), v[..., 0], v[..., 1], v[..., 2], v[..., 3])
    return _TOOL[key]


def miss(far, omax):
    return [0.0, 1000.0 if far else 200.0, -0.9 * omax if far else -50.0]


def aimed(flat, T, s, omax, kind, b, lane, far, beside):
    """origin of the ray of `lane` aimed at block b (direction +z)"""
    c, _ = centres(flat)
    t = BLOCKS[b][lane % len(BLOCKS[b])]
    z0 = -0.9 * omax if far else -50.0
    if kind == "hit":
        dx = 0.2
    elif kind == "d0":
        dx = R
    elif kind == "coarse":
        return [c[t, 0], c[t, 1] + beside, z0]               # between two rows of the lattice (near) / beyond it (far): no sphere within the fine band
    else:
        o0 = np.array([[c[t, 0], c[t, 1], z0]])
        band = float(X.mfma_band(o0, c[t][None], np.array([R]), s)[0])
        for _ in range(3):                                   # (the band moves with |o|: settle the offset on it)
            dx = np.sqrt(R * R + 0.99 * band)
            band = float(X.mfma_band(o0 + [[dx, 0, 0]], c[t][None], np.array([R]), s)[0])
        dx = np.sqrt(R * R + 0.99 * band)
    return [c[t, 0] + dx, c[t, 1], z0]


def build_cases(flat, T, s, omax):
    """-> list of (name, o [m, 3], d [m, 3], aimed cell (half, block) or None, kind, bad lane or None); m = 64, or fewer lanes with a ray"""
    out = []
    for far in (False, True):
        tag = "far" if far else "near"
        beside = 60.0 if far else 1.3
        def wave(kind, h, b, count=64, bad=None):
            o, d = [], []
            for lane in range(count):
                if kind != "none" and lane // 32 == h:
                    o.append(aimed(flat, T, s, omax, kind, b, lane, far, beside))
                else:
                    o.append(miss(far, omax))
                d.append([0.0, 0.0, 1.01] if lane == bad else [0.0, 0.0, 1.0])
            return np.array(o, T).astype(np.float64), np.array(d, T).astype(np.float64)
        out.append((f"{tag}_none", *wave("none", 0, 0), None, "none", None))
        for h in (0, 1):
            for b in range(3):
                for kind in KINDS:
                    name = f"{tag}_{kind}_half{h}_block{b}"
                    out.append((name, *wave(kind, h, b), (h, b), kind, None))
                    bad = 40 if h == 0 else 7                # a ray off the filter in the OTHER half: every sphere is its candidate
                    out.append((name + "_bad", *wave(kind, h, b, bad=bad), (h, b), kind, bad))
                    for count in (20, 40, 48):
                        if count > 32 * h:                   # (the aimed half has lanes with a ray)
                            out.append((name + f"_{count}lanes", *wave(kind, h, b, count=count), (h, b), kind, None))
    return out


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_every_path_of_a_half_block(oracle, T, numerics, tmp_path):
    flat = scene(T)
    cc, rr = centres(flat)
    s = X.mfma_scale(cc, rr)
    _, _, omax = X.mfma_ray_constants(s)
    cases = build_cases(flat, T, s, omax)
    # full waves go through the device in ONE launch per op (a wave = 64 consecutive rays); a wave with fewer lanes must end its launch
    full = [k for k, cs in enumerate(cases) if len(cs[1]) == 64]
    part = [k for k, cs in enumerate(cases) if len(cs[1]) != 64]
    groups = [full] + [[k] for k in part]
    O_all = np.concatenate([cs[1] for cs in cases]); D_all = np.concatenate([cs[2] for cs in cases])
    start = np.cumsum([0] + [len(cs[1]) for cs in cases])
    mok, P1, E1, W, E2 = model(flat, O_all, D_all, tmp_path)
    tmax_all = np.full(len(O_all), np.inf)
    disc, dset, hset = oracle_sets(oracle, flat, O_all, D_all, TMIN, tmax_all, T)
    ref_idx, ref_t = oracle.hit_world_batch(flat, np.concatenate([O_all, D_all], 1).astype(T), T(TMIN), np.inf, T)
    band = X.mfma_band(O_all[:, None, :], cc[None], rr[None], s)
    sD, _, s999 = exact_classes(("two_stage", T), flat, O_all, D_all, band)
    seen = set()
    for k, (name, o, d, cell, kind, bad) in enumerate(cases):
        # the case is what it claims to be, by the exact values alone: the aimed cell takes the intended path, the other half is settled
        rows = slice(start[k], start[k + 1])
        m = len(o)
        use = mok[rows]
        assert np.array_equal(use, np.arange(m) != (-1 if bad is None else bad)), name
        for h in (0, 1):
            lanes = np.arange(m)[(np.arange(m) // 32 == h) & use]
            for b, blk in enumerate(BLOCKS):
                p1, e1, w, e2 = (a[rows][lanes][:, blk.start:blk.stop] for a in (P1, E1, W, E2))
                settled = (p1 + e1 < 0).all()
                opened = (p1 - e1 > 0).any()
                found = (w - e1 - e2 > 0).any()
                nothing = (w + e1 + e2 < 0).all()
                if cell == (h, b) and len(lanes):
                    if kind == "coarse":
                        assert opened and nothing, (name, h, b, float(p1.max()), float(w.max()))
                        seen.add(("coarse", h, b, name.split("_")[0]))
                    else:
                        assert found, (name, h, b, float(w.max()))
                        seen.add(("fine", h, b, name.split("_")[0]))
                elif cell is None or h != cell[0] or not len(lanes):
                    if bad is None or bad // 32 != h:
                        assert settled, (name, h, b, float((p1 + e1).max()) if p1.size else None)
                        seen.add(("settled", h, b, name.split("_")[0]))
        if kind == "d0":
            t = [BLOCKS[cell[1]][lane % len(BLOCKS[cell[1]])] for lane in range(m) if lane // 32 == cell[0]]
            l0 = [lane for lane in range(m) if lane // 32 == cell[0]]
            assert (sD[rows][l0, t] == 0).all(), name                                       # D == 0 exactly
        if kind == "edge":
            t = [BLOCKS[cell[1]][lane % len(BLOCKS[cell[1]])] for lane in range(m) if lane // 32 == cell[0]]
            l0 = [lane for lane in range(m) if lane // 32 == cell[0]]
            assert (sD[rows][l0, t] < 0).all() and (s999[rows][l0, t] > 0).all(), name      # inside the band, near its low edge
    # every path occurs in both halves, at every block position, near the origin and far out
    for path in ("settled", "coarse", "fine"):
        for h in (0, 1):
            for b in range(3):
                for tag in ("near", "far"):
                    assert (path, h, b, tag) in seen, (path, h, b, tag)
    for op in (13, 14):
        for g in groups:
            sel = np.concatenate([np.arange(start[k], start[k + 1]) for k in g])
            o, d = O_all[sel], D_all[sel]
            m = len(sel)
            x = np.concatenate([o, d, np.full((m, 1), float(T(TMIN))), np.full((m, 1), np.inf)], 1)
            y = run_unit(op, x, 9, T, flat=flat)
            wrong = (y[:, 0].astype(np.int64) != ref_idx[sel]) | ((ref_idx[sel] >= 0) & (y[:, 1] != ref_t[sel].astype(np.float64)))
            assert not wrong.any(), (cases[g[0]][0], op, numerics, np.flatnonzero(wrong)[:5], y[wrong][:3, :2], ref_idx[sel][wrong][:3])
            ok, sc, cand, inl = run_sink(op, flat, o, d, float(T(TMIN)), tmax_all[sel], T)
            assert not inl.any() and np.array_equal(ok, mok[sel]), (cases[g[0]][0], op)
            cand = cand[:, :N]
            lost = (hset[sel] if op == 14 else dset[sel]) & ~cand
            assert not lost.any(), (cases[g[0]][0], op, numerics, [(int(a), int(b)) for a, b in zip(*np.nonzero(lost))][:5])
            assert cand[~ok].all(), (cases[g[0]][0], op)                                    # a ray off the filter takes every sphere
            if op == 13:
                must = (s999[sel] > 0) & ok[:, None]
                assert not (must & ~cand).any(), (cases[g[0]][0], op)
                # the device's fine values against the exact ones, wherever those are decisive
                w, e = W[sel], E1[sel] + E2[sel]
                sure, none = (w - e > 0) & ok[:, None], (w + e < 0) & ok[:, None]
                assert not (sure & ~cand).any(), (cases[g[0]][0], [(int(a), int(b)) for a, b in zip(*np.nonzero(sure & ~cand))][:5])
                assert not (none & cand).any(), (cases[g[0]][0], [(int(a), int(b)) for a, b in zip(*np.nonzero(none & cand))][:5])
