"""The block layout of the plain matrix-pipe scan (csrc/rtw_plain_layout.hpp, plain C++) on the CPU: tests/plain_layout_check.cpp, compiled
and run here.  No GPU, no HIP."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "plain_layout_check.cpp")


def build_tool(tmp_dir):
    """-> path of the compiled check program"""
    exe = os.path.join(str(tmp_dir), "plain_layout_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def blocks_of(exe, centres, tmp_dir):
    """the layout builder's answer for `centres` (n x 3): (number of blocks, block of every sphere)"""
    path = os.path.join(str(tmp_dir), "centres.txt")
    with open(path, "w") as f:
        f.write(f"{len(centres)}\n")
        for c in centres:
            f.write(" ".join(repr(float(v)) for v in c) + "\n")
    r = subprocess.run([exe, "--blocks", path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-500:]
    lines = r.stdout.split()
    assert lines[0] == "blocks"
    return int(lines[1]), np.array([int(v) for v in lines[2:]], dtype=np.int64)


def test_plain_layout_on_the_cpu(tmp_path):
    """all centres equal, all on one line, lattices with exact ties, random layers / cubes / far clusters, n = 0, 1, 31, 32, 33, 64, 65,
    96, 97, 484, 1000, 2047: every sphere exactly once, ceil(n / 32) blocks, fills that differ by at most one, the identity for at most
    one block, the same permutation twice; the headline scene's 484 spheres come out as 16 compact patches"""
    exe = build_tool(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "deterministic" in r.stdout, r.stdout[-500:]


def test_blocks_mode_reports_a_partition(tmp_path):
    exe = build_tool(tmp_path)
    rng = np.random.default_rng(5)
    for n in (1, 32, 33, 97):
        c = np.stack([rng.uniform(-8, 8, n), np.full(n, 0.2), rng.uniform(-3, 3, n)], axis=1)
        nb, blk = blocks_of(exe, c, tmp_path)
        assert nb == (n + 31) // 32 and len(blk) == n
        fill = np.bincount(blk, minlength=nb)
        assert fill.sum() == n and fill.max() - fill.min() <= 1 and fill.max() <= 32
