#!/usr/bin/env python3
"""Shared-prefix decode steps: flash_cosine_sim_attention_with_shared_prefix (the prefix cached once; prefix phase + suffix phase + one
merge launch) against the plain flash_cosine_sim_attention_with_kvcache call on caches that each hold a COPY of the prefix in front of the
sequence's own positions -- what a caller had before.  ONE process, the two calls alternated round by round and warm (bf16, causal, scale
8, H 32, Hk 8, D 128, N = 1, own length 256, no append; per-call time of `--steps` back-to-back calls between HIP events; median, with the
min ... max over the rounds as the run-to-run spread).  Each route rotates over enough copies of its caches that consecutive calls read
different memory, at least ROTATE_BYTES of keys and values before a buffer comes round again (more than the 256 MB last-level cache), so
the figures are those of caches coming from HBM, as in a serving step, not cache-warm ones; "copies" says how many (shared / plain).
Before timing, the two results are compared on the same seeded inputs (max |diff| in the table: both round to bf16, the composed route
once more).
"KV MB" is what each route must read at least: the plain call B * (P + own) key and value rows, the shared-prefix call P + B * own.
No threshold is asserted: the file records what was measured, slower shapes included.
usage: decode_prefix_ab.py [--rounds R] [--steps K] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flash_cosine_sim_attention_amd as F  # noqa: E402

DT = torch.bfloat16
H, HK, D, OWN, N = 32, 8, 128, 256, 1
SHAPES = [(B, P) for P in (1024, 8192) for B in (8, 32, 128)]
ROTATE_BYTES = 600e6


def timed(fn, steps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1000.0 / steps


def ab(fns, rounds, steps):
    for f in fns:                                  # warm-up
        f()
        f()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            times[i].append(timed(f, steps))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def rotating(calls):
    """one callable that runs the next of `calls` every time"""
    state = {"i": 0}

    def call():
        out = calls[state["i"] % len(calls)]()
        state["i"] += 1
        return out
    return call


def case(B, P):
    row = HK * D * 2 * 2                           # bytes of one position's key and value rows
    bytes_shared, bytes_plain = (P + B * OWN) * row, B * (P + OWN) * row
    n_shared, n_plain = (max(1, -(-int(ROTATE_BYTES) // b)) for b in (bytes_shared, bytes_plain))
    q = torch.randn(B, H, N, D, device="cuda", dtype=DT)
    own = torch.full((B,), OWN, dtype=torch.int32, device="cuda")
    full = torch.full((B,), P + OWN, dtype=torch.int32, device="cuda")
    plen = torch.tensor([P], dtype=torch.int32, device="cuda")
    pk, pv = (torch.randn(1, HK, P, D, device="cuda", dtype=DT) for _ in range(2))
    kc, vc = (torch.randn(B, HK, OWN, D, device="cuda", dtype=DT) for _ in range(2))
    fk = torch.cat([pk.expand(B, -1, -1, -1), kc], dim=2).contiguous()
    fv = torch.cat([pv.expand(B, -1, -1, -1), vc], dim=2).contiguous()

    def shared_on(pk, pv, kc, vc):
        return lambda: F.flash_cosine_sim_attention_with_shared_prefix(q, pk, pv, kc, vc, prefix_len=plen, cache_seqlens=own, max_seqlen_k=OWN,
                                                                       causal=True)

    def plain_on(fk, fv):
        return lambda: F.flash_cosine_sim_attention_with_kvcache(q, fk, fv, cache_seqlens=full, max_seqlen_k=P + OWN, causal=True)

    # copy 0 holds the same values on both routes (the comparison before timing); the further copies are clones: same values, other memory
    shared = [shared_on(pk, pv, kc, vc)] + [shared_on(pk.clone(), pv.clone(), kc.clone(), vc.clone()) for _ in range(n_shared - 1)]
    plain = [plain_on(fk, fv)] + [plain_on(fk.clone(), fv.clone()) for _ in range(n_plain - 1)]
    diff = float((shared[0]().float() - plain[0]().float()).abs().max())
    return rotating(shared), rotating(plain), bytes_shared, bytes_plain, n_shared, n_plain, diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_prefix_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_prefix_ab.py measures on the GPU: no GPU visible")
    lines = [f"# tools/decode_prefix_ab.py --rounds {a.rounds} --steps {a.steps}: bf16, causal, scale 8, H{H} Hk{HK} D{D}, N = {N}, own length {OWN}, "
             "no append; us per call: median (min ... max over the rounds); every route rotates over `copies` sets of caches "
             f"(>= {ROTATE_BYTES / 1e6:.0f} MB of keys and values between two uses of a buffer: HBM-resident, not cache-warm)",
             f"# device: {torch.cuda.get_device_name(0)}",
             f"{'shape':12s} {'KV MB shared':>12s} {'KV MB plain':>11s} {'copies':>7s} {'shared-prefix us':>32s} {'plain (prefix copies) us':>32s} {'speed-up':>9s} "
             f"{'plain spread':>12s} {'max |diff|':>10s}"]
    torch.manual_seed(0)
    fmt = lambda t: f"{t[0]:9.1f} ({t[1]:.1f} ... {t[2]:.1f})"
    with torch.no_grad():
        for B, P in SHAPES:
            shared, plain, mb_s, mb_p, n_s, n_p, diff = case(B, P)
            t_s, t_p = ab([shared, plain], a.rounds, a.steps)
            note = "" if t_s[0] <= t_p[0] else "   (slower than the plain call)"
            lines.append(f"{f'B{B} P{P}':12s} {mb_s / 1e6:12.1f} {mb_p / 1e6:11.1f} {f'{n_s}/{n_p}':>7s} {fmt(t_s):>32s} {fmt(t_p):>32s} {t_p[0] / t_s[0]:8.2f}x "
                         f"{100 * (t_p[2] - t_p[1]) / t_p[0]:11.1f}% {diff:10.2e}{note}")
            print(lines[-1], flush=True)
            del shared, plain
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
