#!/usr/bin/env python3
"""Compare kernels of two gfx950 assembly listings (hipcc -save-temps: *-hip-amdgcn-amd-amdhsa-gfx950.s) instruction for instruction.

    python tools/isa_compare.py PARENT.s NEW.s [name-substring ...]

Every function of PARENT.s whose mangled name contains one of the substrings (default: every function) must be in NEW.s with the same
instructions in the same order; comments and directives are dropped and the function's own number in local labels (.LBB<n>_<k>) is
normalised, since it only counts the functions in front of it.  Prints one line per function and exits 1 on any difference."""
import re
import sys


def functions(path):
    out, name = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        s = line.split(";")[0].strip()
        if not s or (s.startswith(".") and not s.startswith(".LBB")):
            continue
        out[name].append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    a, b = functions(argv[1]), functions(argv[2])
    keys = argv[3:]
    bad = 0
    for name in sorted(a):
        if keys and not any(k in name for k in keys):
            continue
        same = a[name] == b.get(name)
        bad += not same
        print(f"{name}: {len(a[name])} instructions and labels, {'the same' if same else 'DIFFERENT'}")
    new = sorted(n for n in b if n not in a)
    for name in new:
        print(f"{name}: {len(b[name])} instructions and labels, new")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
