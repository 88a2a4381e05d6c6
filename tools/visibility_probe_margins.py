"""The record of the visibility probe (tests/visibility_probe.py): per dtype and quantity the derived bar and the worst measured ratio to it
from a tolerance log of tests/test_gpu_visibility_probe.py (tests/tolerances.py, FCSA_TOL_LOG; other tests' lines are skipped), then the
(case, quantity) pairs that cannot decide a single pair, by name, as tests/test_visibility_probe_cpu.py computes them (no GPU).
usage: python tools/visibility_probe_margins.py tol_log.jsonl > profiles/visibility_probe_margins.txt"""
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    import test_visibility_probe_cpu as C
    worst = collections.defaultdict(lambda: [0, 0.0, None, 0.0])      # n, ratio, case, bar
    for fn in sys.argv[1:]:
        for line in open(fn):
            r = json.loads(line)
            if not r["label"].startswith("probe/"):
                continue
            _, quantity, call = r["label"].split("/")
            w = worst[r["dtype"], quantity]
            w[0] += 1
            ratio = r["measured"] / r["bar"]
            if ratio >= w[1]:
                w[1], w[2], w[3] = ratio, f"{r['case']} ({call})", r["bar"]
    print("bars: o 2 eps, dq / dk / dv 4 eps of the terms' absolute sum (float32: the rtol of tests/tolerances.py); lse: measured / (4 eps_f32 max(1, |lse|))")
    print("%-5s %-4s %6s %11s %9s  %s" % ("dtype", "qty", "n", "bar", "max m/bar", "worst case"))
    for (dt, q), (n, ratio, case, b) in sorted(worst.items()):
        print("%-5s %-4s %6d %11.3e %9.3f  %s" % (dt, q, n, b, ratio, case))
    print()
    print(f"(case, quantity) pairs that cannot decide a single pair (cap {C.CAP:.0%} of a table; still compared at the bar):")
    print("  o and dv: rows that see more keys than the dtype's bits separate (~1 / (1.5 bar) per feature).  dq: its bar is relative to the sum of the")
    print("  ABSOLUTE terms, so a flip is lost where one term dominates the element it lands in -- a key that shares its feature 1 + j % (D - 1) with")
    print("  the row's diagonal key (under a key mask), or a row at a band's corner that sees no key of its own class (dS = 0).  dk has no single-pair")
    print("  claim of its own: it is the transpose sum of the same dS that dq decides, and dv covers the joint dK/dV kernels.")
    for table in sorted(C.TABLES):
        rows = C.TABLES[table]()
        bad = [(n, q) for n, q, ok in rows if not ok]
        print(f"{table}: {len(bad)} of {len(rows)}")
        for n, q in bad:
            print(f"  {n} {q}")


if __name__ == "__main__":
    main()
