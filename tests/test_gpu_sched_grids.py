"""The trace kernel's job scheduler under small launch grids (csrc/rtw_kernels.hpp claim_job, open_job, the slot protocol of the lane loop;
DESIGN.md section 7.17).  At the natural grid a small frame gives every workgroup a handful of single-position claims; capped at 1 .. 64
workgroups (RTW_GRID_BLOCKS under RTW_ENABLE_TEST_AIDS=1, csrc/rtw_launch.hip job_shape) the same frame is for the scheduler what 1080p is
at the natural grid: guided claims of 8 tapering to 1 handed out of the LDS cache, refills under the lock with four waves of one workgroup
contending for it, queues without a home workgroup (tests/sched_cases.py, tests/test_sched_cases.py: the census of these regimes).

One test per cap, 0 = no cap (the control).  The aids are read once per process, so each test starts ONE fresh child process -- this file
run as a script -- that runs every case of the table through the C ABI (plain, sharded, compact, batched, progressive, adaptive, batched
adaptive; A - C three times each: the hand-out order is not deterministic) and prints one JSON line per run: the sha256 of the image
bytes and the counters.  The parent compares them with references computed on the CPU, once per module: the oracle's renders (masked to
a shard's tiles, view by view for a batch), its segment counts, and for the adaptive case the witness of tests/test_gpu_adaptive.py --
the stopping rule applied to the oracle's samples.  A job rendered twice or lost changes an image, a sample count or a segment count.
Tolerance: NONE -- bits and exact integers.

A child that ends by a signal, an abort, its time limit or an error is a finding about the scheduler: every later parametrisation then
fails at once without starting a process.  Time limits: four times the child's wall time measured on an MI355X, at least
120 s (the margin is for a cold start of torch and the library)."""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import sched_cases as S

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CHECKS = [16, 32, 48]                                       # the checkpoints of the adaptive case (tests/test_gpu_adaptive.py)
GOLDEN48 = "cfg2_random_320x180_64spp_d16_f32"              # its scene and first camera

#: seconds.  Measured wall time of a child on an MI355X, the start of torch and the library included: 2.3 s without a cap, 5.1 / 3.2 / 2.7 /
#: 2.7 / 2.5 / 2.7 s at the caps 1 / 3 / 8 / 9 / 24 / 64 (the cases alone: 0.29 s, 2.98 ... 0.24 s).  Four times the slowest is 20 s: the floor holds
CHILD_LIMIT = {cap: 120 for cap in (0,) + S.G}

_dead = []          # a child ended by signal, abort, time limit or error: (cap, what) -- no further child is started


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _cam_dict(cam):
    return {k: getattr(cam, k) for k in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w", "lens_radius")}


def _random_scene(R, T):
    R.reseed()
    return R.flatten_scene(R.scene_random_spheres(elem_type=T), T)


def _compact_pixels(R, img, idx, cnt):
    """the in-image pixels of a compact shard buffer, in buffer order (`img`: the buffer as gpu_render returns it, a frame-shaped view)"""
    where = R.compact_to_frame_index(S.A["width"], idx, cnt)
    flat = np.ascontiguousarray(img.transpose(1, 0, 2)).reshape(-1, 3)
    return flat[:where.size][where >= 0]


def _other_shards():
    return [(i, cnt) for idx, cnt in S.B["shards"] for i in range(cnt) if i != idx]


# ---- the child: every case of the table, one JSON line per run ----------------------------------------------------------------------------
def _child(tol):
    import torch
    torch.cuda.init()                       # (two HIP runtimes in one process: torch's goes first, tests/conftest.py)
    import rtw_amd as R
    from conftest import CamObj, load_golden
    from test_gpu_accum import Acc
    from test_gpu_accum_batch import batch_adapt
    from test_gpu_adaptive import DEPTH, SEED, SPP, Ad
    from test_gpu_batch import batch
    from test_gpu_render import gpu_render
    t0 = time.time()

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    def counters(st):
        return dict(samples=int(st.samples), segments=int(st.segments), grid_blocks=int(st.grid_blocks))

    # A, B: the 112 x 63 frame
    for T in (np.float32, np.float64):
        flat, cam = _random_scene(R, T), _cam_dict(R.t_cam1(elem_type=T))
        rows = S.A["rows"] if T is np.float32 else S.A["rows"][:S.A["f64_rows"]]
        for jp, spp, nch in rows:
            g = dict(flat=flat, cam=cam, image=np.zeros(1, T), width=S.A["width"], height=S.A["height"], spp=spp, depth=S.A["depth"],
                     seed=S.A["seed"], n_chunks=nch)
            for flags in S.A["flags"]:
                for run in range(S.A["repeats"]):
                    img, st = gpu_render(g, flags=flags, job_pixels=jp)
                    emit(case="A", key=[T.__name__, jp, flags], run=run, sha=_sha(img), **counters(st))
            if T is np.float32 and (jp, spp, nch) == S.B["row"]:
                for idx, cnt in S.B["shards"]:
                    for layout in S.B["layouts"]:
                        for run in range(S.B["repeats"]):
                            img, st = gpu_render(g, flags=layout, job_pixels=jp, shard_index=idx, shard_count=cnt)
                            emit(case="B", key=[idx, cnt, layout], run=run, sha=_sha(_compact_pixels(R, img, idx, cnt) if layout else img), **counters(st))
                for idx, cnt in _other_shards():
                    img, st = gpu_render(g, flags=0, job_pixels=jp, shard_index=idx, shard_count=cnt)
                    emit(case="B", key=[idx, cnt, 0], run=0, sha=_sha(img), **counters(st))
    # C: the batch
    T = np.float32
    flat = _random_scene(R, T)
    cams = [R.t_cam1(elem_type=T), R.t_cam2(elem_type=T), R.t_default_cam(elem_type=T)]
    for jp in S.C["job_pixels"]:
        for run in range(S.C["repeats"]):
            imgs, st = batch(flat, cams, list(S.C["seeds"]), T, S.C["width"], S.C["height"], S.C["spp"], S.C["depth"], S.C["n_chunks"], job_pixels=jp)
            emit(case="C", key=[jp], run=run, sha=[_sha(im) for im in imgs], **counters(st))
    # D: passes into one accumulator, the running image on the last
    jp, spp, nch = S.D["row"]
    a = Acc(flat, R.t_cam1(elem_type=T), T, S.A["width"], S.A["height"], spp, S.A["depth"], S.A["seed"], nch)
    try:
        d_img = torch.full((S.A["width"] * S.A["height"] * 3,), -1.0, dtype=torch.float32, device="cuda:0")
        for k, (b, c) in enumerate(S.D["passes"]):
            st = a.add_ok(b, c, job_pixels=jp, d_out=d_img.data_ptr() if k == len(S.D["passes"]) - 1 else None)
            emit(case="D", key=[b, c], run=0, chunk_spp=a.chunk_spp, **counters(st))
        torch.cuda.synchronize()
        running = d_img.cpu().numpy().reshape(S.A["width"], S.A["height"], 3).transpose(1, 0, 2)
        emit(case="D", key=["end"], run=0, sha=_sha(running), sha_resolved=_sha(a.resolve()))
    finally:
        a.close()
    # E: the adaptive case, one view and a batch of two
    g = load_golden(GOLDEN48, numerics="reference")
    cams = [CamObj(g["cam"]), R.t_cam2(elem_type=T)]
    views = [Ad(g["flat"], cams[v], T, S.E["width"], S.E["height"], SPP, DEPTH, S.E["seeds"][v], n_chunks=SPP, min_chunks=16, check_chunks=16) for v in (0, 0, 1)]
    try:
        assert (S.E["seeds"][0], S.E["first_chunks"]) == (SEED, 16)
        views[0].run_ok(tol, job_pixels=S.E["job_pixels"])
        st_single = counters(views[0].stats())
        views[1].C.check(batch_adapt(views[1:], tol, job_pixels=S.E["job_pixels"]))
        st_batch = counters(views[1].stats())
        for name, a, st in (("single", views[0], st_single), ("batch0", views[1], st_batch), ("batch1", views[2], st_batch)):
            ai = a.ainfo()
            emit(case="E", key=[name], run=0, sha=_sha(a.resolve()), sha_chunks=_sha(a.chunks().astype(np.int32)), sha_words=_sha(a.words()),
                 passes=int(ai["rounds"]), ainfo_samples=int(ai["samples"]), **st)
    finally:
        for a in views:
            a.close()
    emit(case="done", seconds=round(time.time() - t0, 2))


# ---- the parent -----------------------------------------------------------------------------------------------------------------------------
_cache = {}


def _references(oracle, rtw):
    """everything the children are compared with, from the CPU oracle alone; computed once"""
    if _cache:
        return _cache
    from conftest import load_golden
    from rtw_amd import reference_decisions
    from test_gpu_adaptive import DEPTH, FLOOR, SPP, all_samples, oracle_words, rule_chunks
    W, H = S.A["width"], S.A["height"]
    with oracle.numerics("reference"):
        ref = {}
        # A (and B, D: the same frame)
        for T in (np.float32, np.float64):
            flat, cam = _random_scene(rtw, T), _cam_dict(rtw.t_cam1(elem_type=T))
            for jp, spp, nch in (S.A["rows"] if T is np.float32 else S.A["rows"][:S.A["f64_rows"]]):
                img, st = oracle.render(flat, cam, W, H, spp, T=T, max_depth=S.A["depth"], seed=S.A["seed"], n_chunks=S.effective_chunks(spp, nch)[0])
                ref["A", T.__name__, jp] = dict(img=img, sha=_sha(img), segments=st["segments"], samples=W * H * spp)
        frame = ref["A", "float32", S.B["row"][0]]
        for idx, cnt in list(S.B["shards"]) + _other_shards():
            mask = rtw.owned_pixel_mask(W, idx, cnt)
            assert mask.shape == (H, W)
            where = rtw.compact_to_frame_index(W, idx, cnt)
            ref["B", idx, cnt] = {0: _sha(np.where(mask[..., None], frame["img"], np.float32(0))),
                                  S.FLAG_COMPACT_TILES: _sha(np.ascontiguousarray(frame["img"].transpose(1, 0, 2)).reshape(-1, 3)[where[where >= 0]]),
                                  "samples": int(mask.sum()) * S.B["row"][1]}
        # C
        T = np.float32
        flat = _random_scene(rtw, T)
        cams = [rtw.t_cam1(elem_type=T), rtw.t_cam2(elem_type=T), rtw.t_default_cam(elem_type=T)]
        views = [oracle.render(flat, _cam_dict(cam), S.C["width"], S.C["height"], S.C["spp"], T=T, max_depth=S.C["depth"], seed=seed,
                               n_chunks=S.effective_chunks(S.C["spp"], S.C["n_chunks"])[0]) for cam, seed in zip(cams, S.C["seeds"])]
        ref["C"] = dict(sha=[_sha(img) for img, _ in views], segments=sum(st["segments"] for _, st in views),
                        samples=S.C["views"] * S.C["width"] * S.C["height"] * S.C["spp"])
        assert len(set(ref["C"]["sha"])) == S.C["views"]
        # E: the witness of tests/test_gpu_adaptive.py -- the rule on the oracle's samples -- for both views; the tolerance is case48's, picked
        # from view 0's ratios exactly as that fixture picks it
        g = load_golden(GOLDEN48, numerics="reference")
        We, He = S.E["width"], S.E["height"]
        cam_dicts = [g["cam"], _cam_dict(rtw.t_cam2(elem_type=T))]
        wit = []
        for cam, seed in zip(cam_dicts, S.E["seeds"]):
            samples = all_samples(oracle, g["flat"], cam, T, We, He, SPP, DEPTH, seed, SPP)
            words_at = oracle_words(samples, 1, CHECKS + [SPP])
            ratios = {}
            for c in CHECKS:
                _, D, Y, M = reference_decisions(words_at[c], We, He, c, 1.0, FLOOR, return_terms=True)
                ratios[c] = np.array([d / m for d, m in zip(D, M)])
            wit.append(dict(words_at=words_at, ratios=ratios, cam=cam, seed=seed))
        r0 = wit[0]["ratios"]
        allr = np.sort(np.unique(np.concatenate(list(r0.values()))))
        tol, best = None, -1
        for lo, hi in zip(allr[:-1], allr[1:]):
            cand = 0.5 * (lo + hi)
            if min(abs(allr - cand) / cand) <= 1e-6:
                continue
            first = r0[16] <= cand
            never = np.all([r0[c] > cand for c in CHECKS], axis=0)
            score = min(first.sum(), never.sum(), (~first & ~never).sum())
            if score > best:
                tol, best = cand, score
        tol = float(tol)
        tiles_i = (He + 7) // 8
        for w in wit:
            every = np.concatenate(list(w["ratios"].values()))
            assert (np.abs(every - tol) > 1e-9 * tol).all()                   # no ratio near the tolerance: the decisions are not a matter of rounding
            ct = rule_chunks(w["words_at"], CHECKS, SPP, 1, We, He, tol, FLOOR)
            img, words = np.empty((He, We, 3), T), np.empty((He, We, 8), np.uint64)
            for c in sorted(set(ct)):
                prefix, _ = oracle.render(g["flat"], w["cam"], We, He, int(c), T=T, max_depth=DEPTH, seed=w["seed"], n_chunks=int(c))
                for t in np.nonzero(ct == c)[0]:
                    tj, ti = divmod(int(t), tiles_i)
                    img[ti * 8:ti * 8 + 8, tj * 8:tj * 8 + 8] = prefix[ti * 8:ti * 8 + 8, tj * 8:tj * 8 + 8]
                    words[ti * 8:ti * 8 + 8, tj * 8:tj * 8 + 8] = w["words_at"][int(c)][ti * 8:ti * 8 + 8, tj * 8:tj * 8 + 8]
            npix = [min(8, He - 8 * (t % tiles_i)) * min(8, We - 8 * (t // tiles_i)) for t in range(ct.size)]
            w.update(ct=ct, sha=_sha(img), sha_chunks=_sha(ct.astype(np.int32)), sha_words=_sha(words),
                     passes=1 + sum(1 for c in CHECKS if (ct > c).any()), samples=sum(n * int(c) for n, c in zip(npix, ct)),
                     active=tuple(int((ct > c).sum()) for c in CHECKS))
        # the listed passes are the sizes the census counts on, and a real case: tiles stop at the first checkpoint, in between, never
        assert wit[0]["active"] == S.E["listed_single"]
        assert tuple(a + b for a, b in zip(wit[0]["active"], wit[1]["active"])) == S.E["listed_batch"]
        assert len(set(wit[0]["ct"])) >= 3 and wit[0]["sha_chunks"] != wit[1]["sha_chunks"]
        ref["E"] = dict(tol=tol, single=wit[0], batch0=wit[0], batch1=wit[1])
    _cache.update(ref)
    return _cache


def _run_child(cap, tol):
    env = {k: v for k, v in os.environ.items() if not k.startswith("RTW_")}
    env.update(RTW_ENABLE_TEST_AIDS="1", PYTHONPATH=os.pathsep.join([TESTS, ROOT, os.path.join(ROOT, "oracle"), env.get("PYTHONPATH", "")]))
    if cap:
        env["RTW_GRID_BLOCKS"] = str(cap)
    limit = CHILD_LIMIT[cap]
    t0 = time.time()
    try:
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", tol.hex()],
                           env=env, capture_output=True, text=True, timeout=limit + 30, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        _dead.append((cap, f"no end after {limit + 30} s; its output so far:\n{(e.stdout or b'')[-2000:]!r}"))
        pytest.fail(f"child with cap {cap}: {_dead[-1][1]}")
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    print(f"child with cap {cap}: exit {p.returncode}, {time.time() - t0:.1f} s wall, {len(lines)} lines, cases {lines[-1].get('seconds') if lines else None} s")
    if p.returncode != 0 or not lines or lines[-1]["case"] != "done":
        what = "its time limit" if p.returncode in (124, 137) else f"exit status {p.returncode}"
        _dead.append((cap, f"{what}; last line {lines[-1] if lines else None}; stderr:\n{p.stderr[-3000:]}"))
        pytest.fail(f"child with cap {cap} ended by {_dead[-1][1]}")
    return lines[:-1]


@pytest.mark.parametrize("cap", (0,) + S.G)
def test_every_launch_kind_under_a_grid_cap_equals_the_oracle(oracle, rtw, cap):
    if _dead:
        pytest.fail(f"not started: the child with cap {_dead[0][0]} ended by {_dead[0][1]}")
    ref = _references(oracle, rtw)
    _check(cap, _run_child(cap, ref["E"]["tol"]), ref)


def _check(cap, lines, ref):
    """one child's lines against the references"""
    by_case = {c: [ln for ln in lines if ln["case"] == c] for c in "ABCDE"}
    # the aid acted (the control: the natural grid lies above every cap); the issue's regime needs the control's grid above 64
    for ln in lines:
        if "grid_blocks" in ln:
            assert (ln["grid_blocks"] == cap) if cap else (ln["grid_blocks"] > max(S.G)), ln
    # A: plain renders
    assert len(by_case["A"]) == (len(S.A["rows"]) + S.A["f64_rows"]) * len(S.A["flags"]) * S.A["repeats"]
    for ln in by_case["A"]:
        r = ref["A", ln["key"][0], ln["key"][1]]
        assert (ln["sha"], ln["samples"], ln["segments"]) == (r["sha"], r["samples"], r["segments"]), (ln, r["samples"], r["segments"])
    # B: shards; the oracle counts segments per frame: the shards of one count must sum to it, and every run of one shard must agree
    assert len(by_case["B"]) == len(S.B["shards"]) * len(S.B["layouts"]) * S.B["repeats"] + len(_other_shards())
    seg = {}
    for ln in by_case["B"]:
        idx, cnt, layout = ln["key"]
        r = ref["B", idx, cnt]
        assert (ln["sha"], ln["samples"]) == (r[layout], r["samples"]), ln
        assert seg.setdefault((idx, cnt), ln["segments"]) == ln["segments"], ln
    for _, cnt in S.B["shards"]:
        assert sum(seg[i, cnt] for i in range(cnt)) == ref["A", "float32", S.B["row"][0]]["segments"], (cnt, seg)
    # C: the batch, view by view
    assert len(by_case["C"]) == len(S.C["job_pixels"]) * S.C["repeats"]
    for ln in by_case["C"]:
        assert (ln["sha"], ln["samples"], ln["segments"]) == (ref["C"]["sha"], ref["C"]["samples"], ref["C"]["segments"]), ln
    # D: the passes add up to the whole render
    whole = ref["A", "float32", S.D["row"][0]]
    passes, end = by_case["D"][:-1], by_case["D"][-1]
    assert [tuple(ln["key"]) for ln in passes] == list(S.D["passes"]) and end["key"] == ["end"]
    for ln in passes:
        assert ln["samples"] == S.A["width"] * S.A["height"] * ln["chunk_spp"] * ln["key"][1] and ln["chunk_spp"] == 5, ln
    assert sum(ln["segments"] for ln in passes) == whole["segments"]
    assert end["sha"] == whole["sha"] and end["sha_resolved"] == whole["sha"]
    # E: the adaptive runs against the oracle-built witness
    assert [ln["key"][0] for ln in by_case["E"]] == ["single", "batch0", "batch1"]
    for ln in by_case["E"]:
        w = ref["E"][ln["key"][0]]
        assert (ln["sha"], ln["sha_chunks"], ln["sha_words"], ln["passes"], ln["ainfo_samples"]) == (w["sha"], w["sha_chunks"], w["sha_words"], w["passes"], w["samples"]), ln
    single, b0 = by_case["E"][0], by_case["E"][1]
    assert single["samples"] == ref["E"]["single"]["samples"]
    assert b0["samples"] == ref["E"]["batch0"]["samples"] + ref["E"]["batch1"]["samples"]


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(float.fromhex(sys.argv[2]))
