"""The byte arithmetic of the ray queries (csrc/rtw_layout.hpp RaysLayout, rays_grid and the alias ranges of the host form) on the CPU:
tests/rays_layout_check.cpp, a program of its own, compiled here with the host compiler's address and undefined-behaviour sanitizers and
run.  No GPU, no HIP, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "rays_layout_check.cpp")


def test_ray_regions_alias_ranges_and_grid_on_the_cpu(tmp_path):
    """n = 0 .. 2^31 - 1, both element sizes, with and without records: the three regions start on 16-byte boundaries one behind the other
    and share no byte; the alias check names exactly the pairs of the host form that share one; the grid is ceil(n / 256) capped by the
    resident workgroups and by max_workgroups, never below 1, and every batch of 64 rays is walked exactly once under every cap"""
    exe = os.path.join(str(tmp_path), "rays_layout_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "rays layout ok" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])
