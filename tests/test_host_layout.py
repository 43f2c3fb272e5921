"""The byte arithmetic of the host paths (csrc/rtw_layout.hpp, plain C++) on the CPU: tests/host_layout_check.cpp, a program of its own,
compiled here with the host compiler's address and undefined-behaviour sanitizers and run.  No GPU, no HIP, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_layout_check.cpp")
HEADER = os.path.join(ROOT, "raytracingweekend.jl_amd", "csrc", "rtw_layout.hpp")


def test_layout_header_is_plain_cpp():
    """the header includes nothing of HIP and nothing of the library: a host compiler builds it alone"""
    includes = [line.split()[1] for line in open(HEADER) if line.startswith("#include")]
    assert includes and all(i.startswith("<c") for i in includes), includes


def test_regions_and_alias_check_on_the_cpu(tmp_path):
    """frames 1x1, 5x3, 17x33, 96x54, both element sizes, n_views 0 / 1 / 3, workspace sizes that are no multiple of 16: every region of
    the four layouts starts on a 16-byte boundary behind the one before it and `total` reaches the end of the last; the alias check
    reports exactly the pairs that share a byte (disjoint, touching, one byte shared, nested), skips null ranges and names the first
    offending pair in its documented precedence"""
    exe = os.path.join(str(tmp_path), "host_layout_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host layout ok" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])
