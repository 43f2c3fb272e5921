"""The census of the scheduler cases (tests/sched_cases.py), on the model alone: under the grid caps G the inputs of
tests/test_gpu_sched_grids.py reach the regimes of claim_job that the suite's frames do not reach at the natural grid -- guided claims of
4 to 8 positions, queues without a home workgroup, queues shorter and longer than their static part -- and every cap acts.  No GPU,
no kernel: the restated arithmetic only.  `pytest -s` shows the table."""
import sched_cases as S


def _table():
    return [(L, cap, S.census(L, cap)) for L in S.launches() for cap in S.G]


def test_the_arithmetic_by_hand():
    """112 x 63 at one pixel per job: 14 x 8 tiles, queues 0 .. 5 hold 2 x 8 x 64 = 1024 positions and 6, 7 half of that; first guided claims
    of 8 up to 24 workgroups (1024 / (16 x 4) = 16) and of 7 at 64 (1024 / (16 x 9))"""
    q = [S.queue_positions(8, 14, 1, 112, 1, xq) for xq in range(8)]
    assert q == [1024] * 6 + [512] * 2
    assert [S.first_claim(g, 1024) for g in S.G] == [8, 8, 8, 8, 8, 7]
    assert [S.home_workgroups(9, xq) for xq in range(8)] == [2, 1, 1, 1, 1, 1, 1, 1]
    assert [S.home_workgroups(3, xq) for xq in range(8)] == [1, 1, 1, 0, 0, 0, 0, 0]
    assert S.static_claims(64, 0, 1024) == 4 and S.static_claims(64, 0, 20) == 2 and S.static_claims(3, 5, 1024) == 0
    # a shard: local tile k in queue k mod 8 -- shard 4 of 5 holds 22 of the 112 tiles
    assert [S.queue_positions(8, 14, 5, 22, 4, xq) for xq in range(8)] == [48] * 6 + [32] * 2
    assert (S.effective_chunks(130, 130), S.effective_chunks(40, 8), S.effective_chunks(5, 0), S.effective_chunks(17, 6)) == ((130, 1), (8, 5), (5, 1), (6, 3))
    assert [S.useful_grid(112, jp, S.effective_chunks(spp, n)[0]) for jp, spp, n in S.A["rows"]] == [5376, 448, 1120, 224]


def test_census_of_the_cases_under_the_caps():
    table = _table()
    print()
    print(f"{'launch':<22}{'cap':>4}{'grid':>5}  {'first claim of queues 0..7':<28}{'homeless':>9}{'static positions':>18}  queue positions")
    for L, cap, c in table:
        print(f"{L['name']:<22}{cap:>4}{c['grid']:>5}  {' '.join(map(str, c['first'])):<28}{c['homeless']:>9}"
              f"{sum(s * w for s, w in zip(c['static'], c['wgs'])):>18}  {' '.join(map(str, c['q_pos']))}")
    by_cap = {cap: [(L, c) for L, k, c in table if k == cap] for cap in S.G}
    for cap in S.G:
        # a first home-queue claim of at least 4 positions at every cap, of the full 8 up to 9 workgroups
        best = max(max(c["first"]) for _, c in by_cap[cap])
        assert best >= 4, cap
        if cap <= 9:
            assert best == S.RTW_JOB_CLAIM, cap
    for cap in (1, 3):
        assert all(c["homeless"] == 8 - cap for L, c in by_cap[cap] if all(c["q_pos"])), cap       # (every queue has positions: 8 - cap are homeless)
        assert any(all(c["q_pos"]) for _, c in by_cap[cap])
    assert all(c["wgs"] == [2, 1, 1, 1, 1, 1, 1, 1] for _, c in by_cap[9])
    full = S.RTW_STATIC_CLAIMS
    # a queue with positions, but fewer than RTW_STATIC_CLAIMS for each of its workgroups ...
    short = [(L["name"], cap) for L, cap, c in table if any(w and 0 < q < full * w for q, w in zip(c["q_pos"], c["wgs"]))]
    assert short, "no queue shorter than its static part"
    # ... and a launch whose every queue is longer than that, at every cap
    for cap in S.G:
        assert any(all(q > full * w for q, w in zip(c["q_pos"], c["wgs"])) for _, c in by_cap[cap]), cap
    # every cap acts: the launch's useful grid lies above it.  (The listed passes of the adaptive case are its launches over few tiles: 8
    # or 14 tiles of four-pixel jobs are 32 or 56 useful workgroups, below the cap 64 -- there the grid is the smaller of the two, in the
    # model as in job_shape, and the case's FIRST pass, a full frame, carries the claim.)
    for L, cap, c in table:
        if not L["listed"]:
            assert c["useful"] > cap and c["grid"] == cap, (L["name"], cap)
    print("queues shorter than their static part:", short)


def test_the_table_is_the_issues():
    """the cases as specified: nothing dropped"""
    assert S.G == (1, 3, 8, 9, 24, 64)
    assert S.A["rows"] == ((1, 130, 130), (4, 40, 8), (8, 40, 40), (16, 5, 0)) and S.A["flags"] == (0, 1) and S.A["f64_rows"] == 2
    assert (S.A["width"], S.A["height"], S.A["depth"]) == (112, 63, 50)
    assert S.B["shards"] == ((1, 3), (4, 5)) and S.B["layouts"] == (0, 2) and S.B["row"][0] == 4
    assert (S.C["width"], S.C["height"], S.C["views"], S.C["job_pixels"]) == (52, 29, 3, (4, 1)) and len(set(S.C["seeds"])) == 3
    assert S.D["passes"] == ((0, 3), (3, 1), (4, 4)) and S.D["row"] == (4, 40, 8)
    assert (S.E["width"], S.E["height"], S.E["job_pixels"]) == (48, 27, 4)
    assert min(S.A["repeats"], S.B["repeats"], S.C["repeats"]) == 3
    names = [L["name"] for L in S.launches()]
    assert len(names) == len(set(names)) == 4 + 2 + 2 + 3 + 2 * 4
