#!/usr/bin/env python3
"""Instruction-count A/B of two device-assembly builds (hipcc -S --cuda-device-only of the same source file, before / after a change):
for every kernel of the first file, compare its MFMA, LDS, exp, barrier and vector-memory instruction counts (tools/isa_summary.py's
classes) with the second file's; print the kernels that differ and a one-line verdict.  Kernels present in only one file are listed.
usage: isa_ab.py before.s after.s"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_summary import summarize, demangle  # noqa: E402

KEYS = ("mfma", "ds", "exp", "bar", "vmem")


def main(a, b):
    A, B = summarize(a), summarize(b)
    names = demangle(sorted(set(A) | set(B)))
    diff = [k for k in sorted(set(A) & set(B)) if any(A[k][x] != B[k][x] for x in KEYS)]
    only = sorted(set(A) ^ set(B))
    for k in diff:
        print(names[k])
        print("   before", " ".join(f"{x}={A[k][x]}" for x in KEYS))
        print("   after ", " ".join(f"{x}={B[k][x]}" for x in KEYS))
    for k in only:
        print("only in", "before" if k in A else "after", names[k])
    print(f"{os.path.basename(a)}: {len(set(A) & set(B))} kernels compared, {len(diff)} differ in {'/'.join(KEYS)} counts, "
          f"{len(only)} in one file only")
    return 1 if diff or only else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
