"""The trace kernel's job scheduler under small launch grids: the case table of tests/test_gpu_sched_grids.py and a restatement of the
scheduler's ARITHMETIC (csrc/rtw_kernels.hpp claim_job / open_job, csrc/rtw_launch.hip job_shape), written from
their comments.  The restatement serves one purpose, the census of tests/test_sched_cases.py: showing that these inputs, under the grid
caps G, reach the scheduler's regimes -- guided claims of several positions handed out of the LDS cache, queues without a home
workgroup, queues shorter and longer than their static part.  The GPU tests never compare the kernel with it: they compare images and
counters with the CPU oracle.

The scheduler in words.  The frame is cut into 8 x 8 tiles, tile t = tj * tiles_i + ti.  A job is `job_pixels` pixels of one tile (64 /
job_pixels jobs per tile) and its work comes in batches of 64 items = job_pixels pixels x 64 / job_pixels chunks, `bpj` batches per job.
There are 8 queues: in a full frame (and a batch, whose views stand side by side: tiles_j = N x the view's) tile column tj belongs to
queue tj mod 8; in a shard and in a listed pass of an adaptive render local tile k belongs to queue k mod 8.  Workgroup b is at home at
queue b mod 8.  Its first RTW_STATIC_CLAIMS claims are positions it owns without an atomic -- every home workgroup of a queue owns the same
number, min(RTW_STATIC_CLAIMS, positions / workgroups) --, behind them the queue's counter hands out guided claims of
clamp(left / (RTW_CLAIM_TAIL * (grid / 8 + 1)), 1, RTW_JOB_CLAIM) positions, `left` counted from what the workgroup's previous claim saw
(nothing before its first), and a workgroup whose home queue is exhausted visits the others one position at a time."""

RTW_JOB_CLAIM, RTW_CLAIM_TAIL, RTW_STATIC_CLAIMS = 8, 16, 4          # csrc/rtw_kernels.hpp

#: the grid caps (RTW_GRID_BLOCKS under RTW_ENABLE_TEST_AIDS=1); the GPU test adds 0 = no cap, the control
G = (1, 3, 8, 9, 24, 64)

FLAG_GROUP_CULL, FLAG_COMPACT_TILES = 1, 2                          # include/rtw_hip.h


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------
def queue_positions(tiles_i, tiles_j, shard_count, local_tiles, job_pixels, xq):
    """positions of queue xq: its tiles x the jobs of a tile (shard_count 1: a full frame of tiles_i x tiles_j tiles; else `local_tiles`
    tiles of a shard or a list)"""
    if shard_count == 1:
        tiles = len(range(xq, tiles_j, 8)) * tiles_i
    else:
        tiles = len(range(xq, local_tiles, 8))
    return tiles * (64 // job_pixels)


def home_workgroups(grid, xq):
    """workgroups b of the grid with b & 7 == xq"""
    return len(range(xq, grid, 8))


def static_claims(grid, xq, q_pos):
    """static positions of EACH home workgroup of queue xq (the queue's static part is this x home_workgroups)"""
    wgs = home_workgroups(grid, xq)
    return min(RTW_STATIC_CLAIMS, q_pos // wgs) if wgs else 0


def first_claim(grid, q_pos):
    """positions a workgroup asks for with its first guided claim on its home queue (it has seen nothing of the queue yet)"""
    return max(1, min(RTW_JOB_CLAIM, q_pos // (RTW_CLAIM_TAIL * (grid // 8 + 1))))


def effective_chunks(spp, n_chunks):
    """(chunks, samples per chunk) of a render: n_chunks 0 = min(spp, 256); chunks that would be empty are dropped"""
    n = n_chunks if n_chunks > 0 else min(spp, 256)
    cs = -(-spp // n)
    return -(-spp // cs), cs


def useful_grid(tiles, job_pixels, n_chunks):
    """the grid beyond which workgroups would find no batch: one batch per wave, four waves per workgroup"""
    jobs = tiles * (64 // job_pixels)
    cpb = 64 // job_pixels
    return (jobs * (-(-n_chunks // cpb)) + 3) // 4


# ---- the cases (the issue's table; every GPU child runs all of them) -------------------------------------------------------------------
#: A -- scene_random_spheres / t_cam1 at 112 x 63 = 14 x 8 tiles: queues 0 .. 5 own two tile columns, 6 and 7 one; a ragged last tile row
A = dict(width=112, height=63, depth=50, seed=1,
         rows=((1, 130, 130), (4, 40, 8), (8, 40, 40), (16, 5, 0)),      # (job_pixels, spp, n_chunks): 3, 1, 5, 2 batches per job
         flags=(0, FLAG_GROUP_CULL), f64_rows=2, repeats=3)
#: B -- shards of A's frame, row (4, 40, 8): (index, count), each in the full-frame layout and compact.  The other shards
#: of both counts run once as well (full-frame layout): the oracle counts segments per frame, so the shards' sum is what can be compared
B = dict(row=(4, 40, 8), shards=((1, 3), (4, 5)), layouts=(0, FLAG_COMPACT_TILES), repeats=3)
#: C -- a batch of 3 views at 52 x 29 (7 x 4 tiles a view: a division by 7 and by a power of two, view borders inside a queue's column
#: run): t_cam1, t_cam2, t_default_cam over scene_random_spheres with their own seeds
C = dict(width=52, height=29, views=3, seeds=(3, 11, 1234567), spp=20, n_chunks=20, depth=16, job_pixels=(4, 1), repeats=3)
#: D -- A's row (4, 40, 8) as passes (begin, count) into one accumulator, the running image on the last
D = dict(row=(4, 40, 8), passes=((0, 3), (3, 1), (4, 4)))
#: E -- the 48 x 27 case of tests/test_gpu_adaptive.py (its tolerance, floor and checkpoints) at job_pixels 4: one view, and a batch of
#: two (the golden camera with seed 7, t_cam2 with seed 18).  `listed`: the tiles still active at the checkpoints 16, 32, 48 -- what the
#: rule gives on the ORACLE's samples (the GPU test asserts these numbers on its witness); they size the listed passes of the census
E = dict(width=48, height=27, job_pixels=4, first_chunks=16, seeds=(7, 18), listed_single=(17, 14, 8), listed_batch=(41, 36, 25))


def _tiles(width, height, views=1):
    return (height + 7) // 8, (width + 7) // 8 * views


def launches():
    """every kernel launch of the table as the scheduler sees it -> dicts: name, tiles_i, tiles_j, shard_count (1: full frame; else the
    queues run over `local_tiles`), local_tiles, job_pixels, n_chunks (of the launch), listed (a pass over a tile list: the few-tile launches,
    whose natural grid may lie below a cap)"""
    out = []
    ti, tj = _tiles(A["width"], A["height"])

    def add(name, tiles_i, tiles_j, shard_count, local_tiles, job_pixels, n_chunks, listed=False):
        out.append(dict(name=name, tiles_i=tiles_i, tiles_j=tiles_j, shard_count=shard_count, local_tiles=local_tiles,
                        job_pixels=job_pixels, n_chunks=n_chunks, listed=listed))

    for jp, spp, nch in A["rows"]:
        add(f"A jp{jp} spp{spp}", ti, tj, 1, ti * tj, jp, effective_chunks(spp, nch)[0])
    jp, spp, nch = B["row"]
    for idx, cnt in B["shards"]:
        add(f"B shard {idx}/{cnt}", ti, tj, cnt, len(range(idx, ti * tj, cnt)), jp, effective_chunks(spp, nch)[0])
    ci, cj = _tiles(C["width"], C["height"], C["views"])
    for jp in C["job_pixels"]:
        add(f"C jp{jp}", ci, cj, 1, ci * cj, jp, effective_chunks(C["spp"], C["n_chunks"])[0])
    jp = D["row"][0]
    for b, c in D["passes"]:
        add(f"D pass [{b},+{c})", ti, tj, 1, ti * tj, jp, c)
    for label, views, listed in (("E single", 1, E["listed_single"]), ("E batch", 2, E["listed_batch"])):
        ei, ej = _tiles(E["width"], E["height"], views)
        add(f"{label} first", ei, ej, 1, ei * ej, E["job_pixels"], E["first_chunks"])
        for n in listed:
            add(f"{label} list {n}", ei, ej, 0, n, E["job_pixels"], E["first_chunks"], listed=True)
    return out


def census(launch, cap):
    """the scheduler's regime of one launch under one cap -> dict: grid (the cap, or the launch's useful grid if that is smaller),
    q_pos[8], wgs[8], static[8] (per workgroup), first[8] (the first guided claim of a home workgroup, limited by what the queue holds
    behind its static part; 0 for a queue without home workgroup), homeless (queues with positions and no home workgroup)"""
    n_tiles = launch["tiles_i"] * launch["tiles_j"] if launch["shard_count"] == 1 else launch["local_tiles"]
    useful = useful_grid(n_tiles, launch["job_pixels"], launch["n_chunks"])
    grid = min(cap, useful)
    q_pos = [queue_positions(launch["tiles_i"], launch["tiles_j"], launch["shard_count"], launch["local_tiles"], launch["job_pixels"], xq)
             for xq in range(8)]
    wgs = [home_workgroups(grid, xq) for xq in range(8)]
    static = [static_claims(grid, xq, q_pos[xq]) for xq in range(8)]
    first = [min(first_claim(grid, q_pos[xq]), q_pos[xq] - static[xq] * wgs[xq]) if wgs[xq] else 0 for xq in range(8)]
    return dict(grid=grid, useful=useful, q_pos=q_pos, wgs=wgs, static=static, first=first,
                homeless=sum(1 for xq in range(8) if q_pos[xq] and not wgs[xq]))
