"""Hand-made waves for the candidate lists of the closest-hit scans (tests/test_list_cases.py on the CPU, tests/test_gpu_list_caps.py on
the GPU), and a restatement of the RULES by which a full list is resolved early, written from the kernels' source.  A helper module,
not a conftest.py.

The five places (csrc/rtw_scan.hpp RTW_FLUSH_*):
  A  hit_world_mfma, block loop        a block records one ENTRY per recording lane with a candidate; in front of that, if
                                       total + 64 > cap (160 entries), the list is resolved and total = 0.  So: a flush when a block
                                       records while 97 or more entries wait.
  B  hit_world_mfma, in-lane filter    the same condition when a filter-class member of the group cull's in-lane list records (Float32)
  C  resolve_pairs_impl, explode loop  entries are exploded into singles 64 entries at a time, one BIT of every entry per iteration; in
                                       front of an iteration that has a bit left, if total + 64 > cap2 (192 singles), the singles are
                                       tested and total = 0.  So: a flush when an iteration starts while 129 or more singles wait.
  D  hit_world (VALU)                  per word of 32 spheres every lane appends its candidates; when some lane would exceed
                                       RTW_LIST_CAP = 16 the lanes push one candidate per trip, and a trip that starts while some lane
                                       holds 16 resolves ALL lists first.  So: 16 candidates in a lane never flush, the 17th does.
  E  hit_world_cull                    lane-local: a push onto a list of 16 resolves that lane's list first: (k - 1) // 16 flushes for
                                       a lane with k >= 1 candidates.
A recording lane (H, j) of a block holds spheres 16 H .. 16 H + 15 of the block for the rays j and j + 32: its entry carries bit
b = ray half << 4 | register for sphere 32 block + 16 H + register.  The explode loop takes the bits of an entry from the LARGEST b down.

Geometry.  Every ray runs along +z from z = -50.  `lines` cases: lane l has its own line, x = 10 (l % 8 + 1), y = 10 (l // 8 + 1); a
sphere of radius 0.5 sits ON the line of the one ray that shall have it as a candidate (its owner) or on a parking line no ray uses
(owner -1); the other lines are >= 10 away: D = 0.25 - 100 or less, against filter bands of the order of 0.01.  So the incidence
matrix (ray x caller's index) is free, and the index decides block, half and register.  `bundle` cases: all rays within 0.1 of one
axis and every sphere on that axis -- every sphere is every ray's candidate.  The closest hit of a ray is its sphere with the smallest z.
Lanes beyond `count` have no ray (the unit kernel gives them a ray along the z axis through the origin, which no sphere is near)."""
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracingweekend.jl_amd", "csrc")
#: what the cases rest on; tests/test_list_cases.py reads them back from the headers
PAIR_CAP, CAP, CAP2, LIST_CAP = 512, 160, 192, 16
PITCH, RADIUS, Z0, TMIN = 10.0, 0.5, -50.0, 1e-3
PARK = (9 * PITCH, 9 * PITCH)
AXIS = (100.0, 100.0)
COUNTS = (64, 40)


def source_caps():
    """(RTW_PAIR_CAP, cap, cap2, RTW_LIST_CAP) as the headers state them"""
    mf = open(os.path.join(CSRC, "rtw_scan_mfma.hpp")).read()
    sc = open(os.path.join(CSRC, "rtw_scan.hpp")).read()
    pair = int(re.search(r"#define RTW_PAIR_CAP (\d+)\b", mf).group(1))
    a = re.search(r"unsigned cap = (\d+) \* RTW_PAIR_CAP / (\d+);", mf)
    b = re.search(r"unsigned cap2 = (\d+) \* RTW_PAIR_CAP / (\d+);", mf)
    lst = int(re.search(r"#define RTW_LIST_CAP (\d+)\b", sc).group(1))
    return pair, int(a.group(1)) * pair // int(a.group(2)), int(b.group(1)) * pair // int(b.group(2)), lst


def line_of(lane):
    return (PITCH * (lane % 8 + 1), PITCH * (lane // 8 + 1))


class Case:
    """name; count (live lanes); owner [n] (lines: the lane, -1 parked; bundle: ignored), z [n], r [n], kind "lines" / "bundle";
    exact / at_least: flush counts claimed for the plain ops (A, B, C: op 13; D: op 10) -- the model must agree; pair: (kind, 0 / 1) for a
    boundary case; tie: True where copies of the closest sphere are planted"""

    def __init__(self, name, count, owner, z=None, r=None, kind="lines", exact=None, at_least=None, pair=None, tie=False):
        self.name, self.count, self.kind = name, count, kind
        self.owner = np.asarray(owner, np.int64)
        self.n = len(self.owner)
        if z is None:                                    # by the caller's index: the first sphere of a line is its closest, whatever the other lines hold
            z = 0.25 * np.arange(self.n)
        self.z = np.asarray(z, np.float64)
        self.r = np.full(self.n, RADIUS) if r is None else np.asarray(r, np.float64)
        self.exact, self.at_least, self.pair, self.tie = exact or {}, at_least or {}, pair, tie
        assert self.n <= 512 and ((self.owner >= -1) & (self.owner < count)).all(), name

    def scale(self, T):
        return 1.0 + 2.0 ** -40 if T is np.float64 else 1.0          # Float64: coordinates that binary32 does not hold

    def centres(self, T):
        c = np.zeros((self.n, 3))
        for i, l in enumerate(self.owner):
            c[i, :2] = AXIS if self.kind == "bundle" else (PARK if l < 0 else line_of(int(l)))
        c[:, 2] = self.z
        return c * self.scale(T)

    def flat(self, T):
        from test_gpu_filters import make_flat
        return make_flat(self.centres(T), self.r * self.scale(T), T)

    def rays(self, T):
        o = np.zeros((self.count, 3))
        for l in range(self.count):
            o[l] = [AXIS[0] + 0.01 * (l % 8), AXIS[1] + 0.01 * (l // 8), 0.0] if self.kind == "bundle" else [*line_of(l), Z0]
        o = (o * self.scale(T)).astype(T).astype(np.float64)
        return o, np.tile([0.0, 0.0, 1.0], (self.count, 1))

    def incidence(self):
        """the design: [count, n], ray x caller's index"""
        if self.kind == "bundle":
            return np.ones((self.count, self.n), bool)
        return self.owner[None, :] == np.arange(self.count)[:, None]

    def copies(self, winners):
        """per ray: the caller's indices of the exact copies of its closest sphere `winners[ray]` (-1: none), ascending"""
        key = np.concatenate([self.centres(np.float32), self.r[:, None]], 1)
        return [[] if w < 0 else [int(i) for i in np.flatnonzero((key == key[w]).all(1))] for w in winners]


# ---- the rules --------------------------------------------------------------------------------------------------------------------
def model_mfma(inc, cap=CAP, cap2=CAP2, exact=(), inlane=()):
    """hit_world_mfma on a wave: inc [64, P] in DEVICE order (rows of lanes without a ray: empty); `exact` positions are tested in-lane
    and never listed, `inlane` positions (in list order) record one entry per candidate lane in front of the block loop.
    -> (A, B, C, when): when[(ray, position)] = (resolve, test_singles call, round of 64 exact tests), each counted over the scan"""
    inc = np.asarray(inc, bool)
    P = inc.shape[1]
    skip = set(exact) | set(inlane)
    st = dict(A=0, B=0, C=0, res=0, call=0, rnd=0)
    when, entries = {}, []

    def test(singles):
        for k, key in enumerate(singles):
            when[key] = (st["res"], st["call"], st["rnd"] + k // 64)
        st["rnd"] += -(-len(singles) // 64)
        st["call"] += 1

    def resolve():
        singles = []
        for p0 in range(0, len(entries), 64):
            chunk = [list(e) for e in entries[p0:p0 + 64]]
            while True:
                act = [e for e in chunk if e]
                if not act:
                    break
                if len(singles) + 64 > cap2:
                    st["C"] += 1
                    test(singles)
                    singles = []
                singles += [e.pop(0) for e in act]
        test(singles)
        st["res"] += 1
        del entries[:]

    for pos in inlane:
        lanes = [l for l in range(64) if inc[l, pos]]
        if lanes:
            if len(entries) + 64 > cap:
                st["B"] += 1
                resolve()
            entries.extend([(l, pos)] for l in lanes)
    for blk in range(-(-P // 32)):
        rec = []
        for L in range(64):
            H, j = L >> 5, L & 31
            bits = []
            for b in range(31, -1, -1):                                   # (the explode loop's order: the largest b first)
                ray, pos = j + 32 * (b >> 4), 32 * blk + 16 * H + (b & 15)
                if pos < P and pos not in skip and inc[ray, pos]:
                    bits.append((ray, pos))
            if bits:
                rec.append(bits)
        if rec:
            if len(entries) + 64 > cap:
                st["A"] += 1
                resolve()
            entries.extend(rec)
    resolve()
    return st["A"], st["B"], st["C"], when


def model_valu(inc, cap=LIST_CAP):
    """hit_world on a wave: inc [64, n] in the scan's order -> (D, when): when[(ray, index)] = the resolve that tests the candidate"""
    inc = np.asarray(inc, bool)
    n = inc.shape[1]
    cnt = np.zeros(64, int)
    held = [[] for _ in range(64)]
    D, res, when = 0, 0, {}

    def resolve():
        nonlocal res
        for l in range(64):
            for i in held[l]:
                when[(l, i)] = res
            held[l] = []
        cnt[:] = 0
        res += 1

    for base in range(0, n, 32):
        m = [list(np.flatnonzero(inc[l, base:base + 32]) + base) for l in range(64)]
        if not any(m):
            continue
        if not any(cnt[l] + len(m[l]) > cap for l in range(64)):
            for l in range(64):
                held[l] += [int(i) for i in m[l]]
                cnt[l] += len(m[l])
            continue
        while any(m):
            if (cnt >= cap).any():
                D += 1
                resolve()
            for l in range(64):
                if m[l]:
                    held[l].append(int(m[l].pop(0)))
                    cnt[l] += 1
    resolve()
    return D, when


def model_cull_valu(order):
    """hit_world_cull: `order` = per lane the candidates in push order -> E per lane (the k-th candidate is tested by resolve k // 16)"""
    return [max(0, (len(o) - 1) // LIST_CAP) for o in order]


def wave_rows(inc):
    """[count, n] -> [64, n]: lanes without a ray have no candidate"""
    out = np.zeros((64, inc.shape[1]), bool)
    out[:len(inc)] = inc
    return out


def huge_of(r):
    """the caller's indices the upload tests in-lane in the plain matrix-pipe scan (csrc/rtw_scene.hip: at most two spheres of radius
    >= 16 x the median, the largest first)"""
    r = np.abs(np.asarray(r, np.float64))
    if len(r) < 8:
        return []
    med = np.sort(r)[len(r) // 2]
    out = []
    for _ in range(2):
        best = -1
        for i in range(len(r)):
            if r[i] >= 16 * med and i not in out and (best < 0 or r[i] > r[best]):
                best = i
        if best < 0:
            break
        out.append(best)
    return out


def big_of(r):
    """the caller's indices of the group cull's BIG class (csrc/rtw_scene.hip build_cull: |r| > 4 x the lower median)"""
    r = np.abs(np.asarray(r, np.float64))
    return [int(i) for i in np.flatnonzero(r > 4 * np.sort(r)[(len(r) - 1) // 2])]


def plain_counts(case):
    """the model's (A, B, C, D) and the two `when` maps of a case under the plain ops 13 and 10 (device order = the caller's order)"""
    inc = wave_rows(case.incidence())
    A, B, C, w13 = model_mfma(inc, exact=huge_of(case.r))
    D, w10 = model_valu(inc)
    return dict(A=A, B=B, C=C, D=D), w13, w10


# ---- the cases --------------------------------------------------------------------------------------------------------------------
MANY = [(0, 255), (128, 255)]          # (in the group cull's order: the last copy of the caller's list is tested resolves after the first / before it)


def _ray(j, flip, count):
    """ray j (0 .. 31) or, in a full wave and when `flip`, its partner of the second half wave: the same recording lanes"""
    return j + 32 if (flip and count == 64) else j


def boundary_A(count, extra):
    """Blocks 0 - 2: every sphere has a recording lane of its own (16 different j per half), so each block records 32 entries: 32, 64,
    96.  The check reads total + 64 > 160, that is total >= 97.  Block 3 is parked but for its first sphere, which is ray 0's when `extra`;
    block 4 holds one sphere of ray 1.  Without the extra block 3 never records and block 4 records at total = 96: no flush.  With it
    block 3 records at 96 (no flush) and block 4 at 97: exactly one.  Singles: 97 or 98, below 129: C = 0."""
    owner = []
    for b in range(3):
        for H in range(2):
            for q in range(16):
                owner.append(_ray((q + 16 * H + 16 * b) % 32, b == 1, count))
    owner += [0 if extra else -1] + [-1] * 31 + [1]
    return Case(f"A_{97 if extra else 96}", count, owner, exact=dict(A=int(extra), B=0, C=0, D=0), pair=("A", int(extra)))


def boundary_C(count, extra, tie=False):
    """Blocks 0 - 3: per half 8 recording lanes with two bits each (registers q and q + 8: ray j and, in a full wave, j + 32): 16 entries
    per block, 64 entries = one chunk of the explode loop, whose two iterations start at total 0 and 64 and leave 128.  Block 4 records at
    64 entries (no A flush) ray 0's sphere 128: the second chunk's first iteration starts at 128 -- 128 + 64 = 192 is not > 192 -- and
    leaves 129.  `extra`: sphere 129 is ray 0's too, a second bit of the same entry: its iteration starts at 129 -> exactly one flush.
    `tie`: spheres 128 and 129 are exact copies in FRONT of ray 0's other spheres: 129 (the larger b) is tested before the flush, 128 after."""
    owner = []
    for b in range(4):
        for H in range(2):
            for q in range(16):
                owner.append(_ray(q % 8 + 8 * H + 16 * (b % 2), q >= 8, count))
    owner += [0, 0 if extra else -1]
    z = None
    if tie:
        z = Case("", count, owner).z + 4.0
        z[128] = z[129] = 0.0
    return Case(("tie_across_C_opposed" if tie else f"C_{129 if extra else 128}"), count, owner, z=z, exact=dict(A=0, B=0, C=int(extra), D=0),
                pair=None if tie else ("C", int(extra)), tie=tie)


DE_LANES = (0, 13, 31, 32, 39)


def boundary_DE(count, extra):
    """Five lanes take turns: sphere 5 k + i is lane DE_LANES[i]'s, k < 16 -- 16 candidates each, the lists are full when the scan ends
    and nothing waits: D = 0, E = 0 in every lane.  `extra`: sphere 80 is lane 13's 17th.  hit_world: after words 0 and 1 lane 13 holds 13;
    word 2 has 3 + 1 more, 13 + 4 > 16, so the lanes push one per trip, and the trip that starts with 16 in lane 13 and its 17th waiting
    resolves all lists: D = 1.  hit_world_cull: lane 13's 17th push finds 16: E = 1 there, 0 elsewhere."""
    owner = [DE_LANES[i] for k in range(16) for i in range(5)] + [13 if extra else -1]
    return Case(f"DE_{17 if extra else 16}", count, owner, exact=dict(A=0, B=0, C=0, D=int(extra)), pair=("DE", int(extra)))


def heavy(count):
    """512 spheres = 16 blocks on the bundle's axis: every ray has 16 candidates per half block.  Pigeonhole: 16 x 64 = 1024 entries, at
    most 160 per resolve: >= 7 resolves, A >= 6 (and A <= 15, one per block at most); count x 512 singles, at most 192 per call of the
    exact tests and A + 1 calls that are no C flush: C >= ceil(count x 512 / 192) - 16; 512 candidates per lane, 16 per resolve: D, E >= 31."""
    s = -(-count * 512 // 192) - 16
    return Case("heavy", count, np.zeros(512, int), z=2.0 * np.arange(512), kind="bundle", at_least=dict(A=6, C=s, D=31, E=31))


B_BIG = {0: 30.0, 5: 3.5, 9: 3.0, 20: 3.0, 33: 20.0, 37: 3.0}


def scene_B(count):
    """Bundle; 32 small spheres ahead on the axis and six large ones around the rays' origins: radii 30 and 20 (>= 16 x the median 0.5:
    huge, exact in-lane) and 3.5, 3, 3, 3 (> 4 x the median: the BIG class, which fits the in-lane list of 8 -- Float32: the filter class).
    Every ray starts inside all six, so each filter member records `count` entries.  64 lanes: 64, 128, and the third finds 128 + 64 > 160:
    one B flush, then 64, 128.  40 lanes: 40, 80, 120, and the fourth flushes.  The three spheres of radius 3 are exact copies and every
    ray's closest hit (it leaves them at t = 3); the last one records behind the flush in both waves.  Float64 has no filter class: B = 0."""
    n = 38
    r = np.full(n, RADIUS)
    z = np.zeros(n)
    k = 0
    for i in range(n):
        if i in B_BIG:
            r[i] = B_BIG[i]
        else:
            z[i] = 10.0 + 2.0 * k
            k += 1
    return Case("B_inlane_filter", count, np.zeros(n, int), z=z, r=r, kind="bundle", tie=True)


def tie_grid(name, count, blocks, g, pattern):
    """Blocks of 16 / g recording lanes per half with g bits each; each ray's spheres in the caller's order are s_0 < s_1 < ...; `pattern`
    picks the two exact copies (z = 0) and the farther sphere (z = 2; every other one lies behind):
      0: copies s_0 and s_last, farther one in the middle      1: copies s_0, s_1, farther s_last      2: farther s_0, copies the last two"""
    owner = []
    per = 16 // g
    for b in range(blocks):
        for H in range(2):
            for q in range(16):
                owner.append(_ray((q // g + per * H + 2 * per * b) % 32, b % 2 == 1, count))
    owner = np.array(owner)
    z = 4.0 + 2.0 * np.arange(len(owner)) / 8.0
    for l in range(count):
        ids = np.flatnonzero(owner == l)
        if len(ids) < 2:
            continue
        if len(ids) == 2:
            z[ids] = 0.0
            continue
        p = (pattern + l) % 3
        a, b2, f = (ids[0], ids[-1], ids[len(ids) // 2]) if p == 0 else (ids[0], ids[1], ids[-1]) if p == 1 else (ids[-2], ids[-1], ids[0])
        z[a] = z[b2] = 0.0
        z[f] = 2.0
    return Case(name, count, owner, z=z, tie=True)


def tie_valu(count):
    """Lanes 3, 36 and 20 have 40 candidates each, interleaved, so the lists fill together and are resolved after every 16th.  Lanes 3 and
    36: the copies are the lane's 1st and 20th candidate (either side of hit_world's first early resolve and of hit_world_cull's); lane 3's
    farther sphere is its 2nd (tested with the first copy, before the second), lane 36's its 40th (after both).  Lane 20: the farther
    sphere is its 1st, the copies its 20th and 40th -- three different resolves, the farther one first."""
    owner = [3, 36, 20] * 40
    z = 4.0 + 2.0 * np.arange(120)
    z[0] = z[3 * 19] = 0.0; z[3] = 2.0
    z[1] = z[3 * 19 + 1] = 0.0; z[3 * 39 + 1] = 2.0
    z[2] = 2.0; z[3 * 19 + 2] = z[3 * 39 + 2] = 0.0
    return Case("tie_across_DE", count, owner, z=z, tie=True)


def tie_many(count, first, last, n=256):
    """Bundle: the spheres `first` .. `last` of the caller's list, but for every eighth one, are ONE sphere (z = 0), every ray's closest; the
    others lie behind.  Coincident centres are nothing a kd split can tell apart, so where the copies land in the group cull's order has
    little to do with the caller's: with every sphere a candidate of every ray the lists are resolved early all the time, and the first
    and the last copy of the caller's list are tested resolves apart, in either order (the GPU test reads the order from op 28)."""
    z = 2.0 + 0.25 * np.arange(n)
    for i in range(first, last + 1):
        if (i - first) % 8 != 3:
            z[i] = 0.0
    return Case(f"tie_many_copies_{first}_{last}", count, np.zeros(n, int), z=z, kind="bundle", tie=True)


def cases(count):
    out = [boundary_A(count, False), boundary_A(count, True), boundary_C(count, False), boundary_C(count, True),
           boundary_DE(count, False), boundary_DE(count, True), heavy(count), scene_B(count), boundary_C(count, True, tie=True),
           tie_grid("tie_one_round", count, 2, 2, 1), tie_grid("tie_rounds_g4", count, 8, 4, 0), tie_grid("tie_rounds_g4_far_first", count, 8, 4, 2),
           tie_grid("tie_resolves_g1", count, 8, 1, 0), tie_grid("tie_resolves_g1_far_first", count, 8, 1, 2), tie_grid("tie_resolves_g2", count, 10, 2, 1),
           tie_valu(count)] + [tie_many(count, a, b) for a, b in MANY]
    assert len({c.name for c in out}) == len(out)
    return out


def classify_ties(case, copies, when, key=lambda ray, i: (ray, i)):
    """per ray with two or more copies (Case.copies): how the model's `when` places the first and the last copy of the caller's list and the ray's
    second-closest sphere -> list of (relation, order, far) with
      relation  "round" (one round of exact tests), "call" (two rounds of one call), "C" (two calls of one resolve), "A" (two resolves);
                for the VALU maps (integers): "round" or "A"
      order     "same", "aligned" (the later copy is tested later) or "opposed"
      far       None, "first+" (a farther sphere of a LARGER index tested strictly before both copies), "first", "after" (strictly after both), "mixed" """
    inc = case.incidence()
    out = []
    for l, cp in enumerate(copies):
        if len(cp) < 2:
            continue
        wa, wb = when[key(l, cp[0])], when[key(l, cp[-1])]
        if isinstance(wa, tuple):
            rel = "A" if wa[0] != wb[0] else "C" if wa[1] != wb[1] else "call" if wa[2] != wb[2] else "round"
        else:
            rel = "A" if wa != wb else "round"
        order = "same" if wa == wb else "aligned" if wa < wb else "opposed"
        others = [int(i) for i in np.flatnonzero(inc[l]) if i not in cp]
        far = None
        if others and case.kind == "lines":
            f = min(others, key=lambda i: case.z[i] - case.r[i])
            wf = when[key(l, f)]
            far = ("first+" if f > cp[-1] else "first") if wf < min(wa, wb) else "after" if wf > max(wa, wb) else "mixed"
        out.append((rel, order, far))
    return out
