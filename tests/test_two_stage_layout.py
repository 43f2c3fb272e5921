"""The two-stage evaluation of the matrix-pipe filter (csrc/rtw_scan_mfma.hpp, "Two stages") on the CPU: tests/two_stage_check.cpp multiplies
the host's sphere operands (csrc/rtw_mfma_operands.hpp, what build_mfma_operands uploads) with a host mirror of the scan prologue's ray
operands in exact integer arithmetic, compiled and run here.  No GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "two_stage_check.cpp")


def test_coarse_value_dominates_the_fine_one(tmp_path):
    """scenes of five scales, spheres out to |c_k| s = 2^8 with radii 1e-3 .. 1e3, k' ~ 0, flat and subnormal coordinates; rays out to the
    filter's |o| limit, tangent rays from near the origin and from 0.9 x the limit, rays off the filter, lanes without a ray, padding rows:
    (a) P1' + P2' is the un-folded 32-product sum up to the fold's documented rounding, (b) P1' - (P1' + P2') >= the bound reserved for
    MFMA 1's accumulation error for every pair on the filter, and D >= 0 implies P1' and W positive with both error bounds to spare,
    (c) every piece a finite binary16 inside its documented range"""
    exe = os.path.join(str(tmp_path), "two_stage_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "P1' - W >= E1 everywhere" in r.stdout, r.stdout[-800:]
