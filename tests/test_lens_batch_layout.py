"""The byte arithmetic of the batched lens stage (csrc/rtw_layout.hpp LensBatchLayout, plain C++) on the CPU: tests/lens_batch_layout_check.cpp,
a program of its own, compiled here with the host compiler's address and undefined-behaviour sanitizers and run, exactly as
tests/test_host_layout.py does.  No GPU, no HIP, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "lens_batch_layout_check.cpp")


def test_strides_extents_and_regions_on_the_cpu(tmp_path):
    """frames 1x1 .. 96x54, both element sizes, max_radius 1 .. 32, 1 .. 7 views of n_views frames or of one: the strides and extents are the
    header's (the workspace restated from its table of regions), every region starts on a 16-byte boundary behind the one before it, and
    the views' bytes, written into a buffer of exactly `total` bytes, never share one"""
    exe = os.path.join(str(tmp_path), "lens_batch_layout_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lens batch layout ok" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])
