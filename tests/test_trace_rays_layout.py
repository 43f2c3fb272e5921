"""The byte arithmetic of the radiance queries (csrc/rtw_layout.hpp TraceRaysLayout, u64_range_wraps, trace_rays_batches, trace_rays_grid
and the alias ranges of the host form) on the CPU: tests/trace_rays_layout_check.cpp, a program of its own, compiled here with the host
compiler's address and undefined-behaviour sanitizers and run.  No GPU, no HIP, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "trace_rays_layout_check.cpp")


def test_trace_ray_regions_ranges_batches_and_grid_on_the_cpu(tmp_path):
    """n = 0 .. 2^31 - 1, both element sizes: the two regions start on 16-byte boundaries one behind the other and share no byte; the alias
    check finds out on the rays by one byte at either end; first + count is refused exactly when it leaves the 64-bit range; every ray
    belongs to exactly one claimed batch under every grid cap"""
    exe = os.path.join(str(tmp_path), "trace_rays_layout_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "trace rays layout ok" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])
