#!/usr/bin/env python3
"""Prompt chunks against a paged key/value cache: flash_cosine_sim_attention_prefill_with_kvcache (the multi-wave kernel of
csrc/fcsa_prefill.hip) against flash_cosine_sim_attention_varlen_with_kvcache (the ragged decode call at its own split count) and, on the
rows that start from an empty cache, against the dense flash_cosine_sim_attention(..., causal=True) forward on the same tokens as the
upper yardstick (contiguous q / k / v, no cache, no append).
ONE process, the routes alternated round by round and warm (bf16, and one float16 D = 128 row -- those instantiations run one wave per
SIMD --, scale 8, pages of 16 through a shuffled block table, every call appends
its tokens; per-call time of `--steps` back-to-back calls between HIP events; median, with the min ... max over the rounds as the
run-to-run spread).  Each cache route rotates over copies of its caches -- at least ROTATE_BYTES of keys and values before a buffer comes
round again (more than the 256 MB last-level cache), at most MAX_COPIES of them -- so the figures are those of caches coming from HBM.
Before timing, the two cache routes are compared on the same inputs (max |diff| in the table; 0 where the ragged call runs one split).
TFLOP/s: the project's convention (bench.py: GEMM FLOPs only, 4 * D per (query head, visible query-key pair)) over the new call's time.
"x ragged" / "x dense" = that route's median time / the new call's: above 1 the new call is faster.  "beyond spread": whether the gap to
the ragged call exceeds the larger of the two routes' min ... max spreads.
No threshold is asserted: the file records what was measured, slower shapes included.
--calls K: no timing, the new call of the selected rows K times each -- the command to put behind `rocprofv3 --pmc ... --`.
usage: prefill_ab.py [--rounds R] [--steps K] [--out FILE] [--only SUBSTRING] [--calls K]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flash_cosine_sim_attention_amd as F  # noqa: E402

DT = torch.bfloat16
PAGE = 16
ROTATE_BYTES = 600e6
MAX_COPIES = 12

# name, H, Hk, D, query counts, cached positions, causal (bf16 unless the name says f16)
ROWS = []
for _cached in (0, 8192, 32768):
    for _n in (64, 256, 1024, 4096):
        ROWS.append((f"N{_n} on {_cached}", 32, 8, 128, [_n], [_cached], True))
for _n in (64, 256, 1024, 4096):
    ROWS.append((f"N{_n} on 0 non-causal", 32, 8, 128, [_n], [0], False))
ROWS.append(("D64 H8/Hk8 N1024 on 8192", 8, 8, 64, [1024], [8192], True))
ROWS.append(("f16 N1024 on 8192", 32, 8, 128, [1024], [8192], True))
ROWS.append(("f16 N4096 on 8192", 32, 8, 128, [4096], [8192], True))
ROWS.append(("8 x N512 on 4096", 32, 8, 128, [512] * 8, [4096] * 8, True))
ROWS.append(("63 x N1 + N512 on 4096", 32, 8, 128, [1] * 63 + [512], [4096] * 64, True))


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


def visible_pairs(counts, cached, causal):
    """query-key pairs a call computes: token i of N against L = cached + N positions sees L (causal: L - N + i + 1) keys"""
    total = 0
    for n, c in zip(counts, cached):
        L = c + n
        total += n * L - (n * (n - 1) // 2 if causal else 0)
    return total


def case(H, Hk, D, counts, cached, causal, DT=DT):
    B, total = len(counts), sum(counts)
    cap = -(-max(c + n for c, n in zip(counts, cached)) // PAGE) * PAGE
    mb = cap // PAGE
    kv_bytes = sum(c + n for c, n in zip(counts, cached)) * Hk * D * 2 * 2
    copies = min(MAX_COPIES, max(1, -(-int(ROTATE_BYTES) // kv_bytes)))
    q = torch.randn(total, H, D, device="cuda", dtype=DT)
    kn, vn = (torch.randn(total, Hk, D, device="cuda", dtype=DT) for _ in range(2))
    cu = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32, device="cuda")
    sl = torch.tensor(cached, dtype=torch.int32, device="cuda")
    table = torch.randperm(B * mb, generator=torch.Generator().manual_seed(1)).to(torch.int32).view(B, mb).cuda()
    kw = dict(cache_seqlens=sl, block_table=table, max_seqlen_q=max(counts), max_seqlen_k=cap, causal=causal)

    def pools():
        return tuple(torch.randn(B * mb, Hk, PAGE, D, device="cuda", dtype=DT) for _ in range(2))

    first = pools()
    sets = [first] + [tuple(t.clone() for t in first) for _ in range(copies - 1)]      # same values, other memory
    new = [(lambda k, v: (lambda: F.flash_cosine_sim_attention_prefill_with_kvcache(q, k, v, cu, kn, vn, **kw)))(k, v) for k, v in sets]
    old = [(lambda k, v: (lambda: F.flash_cosine_sim_attention_varlen_with_kvcache(q, k, v, cu, kn, vn, **kw)))(k, v) for k, v in sets]
    diff = float((new[0]().float() - old[0]().float()).abs().max())
    dense = None
    if all(c == 0 for c in cached):
        n = counts[0]
        qd = q.view(B, n, H, D).transpose(1, 2).contiguous()
        kd, vd = (t.view(B, n, Hk, D).transpose(1, 2).contiguous() for t in (kn, vn))
        dense = lambda: F.flash_cosine_sim_attention(qd, kd, vd, causal=causal)
    return rotating(new), rotating(old), dense, copies, diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", default="")
    ap.add_argument("--calls", type=int, default=0, help="no timing: run the new call of every selected row this many times (under a profiler)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefill_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prefill_ab.py measures on the GPU: no GPU visible")
    lines = [f"# tools/prefill_ab.py --rounds {a.rounds} --steps {a.steps}: bf16 (rows named f16: float16), scale 8, paged cache (pages of {PAGE}, shuffled table), every call "
             "appends its tokens; us per call: median (min ... max over the rounds); the cache routes rotate over `copies` sets of caches "
             f"(>= {ROTATE_BYTES / 1e6:.0f} MB of keys and values between two uses of a buffer, at most {MAX_COPIES} sets)",
             f"# device: {torch.cuda.get_device_name(0)}",
             f"{'row':28s} {'copies':>6s} {'Mpairs':>8s} {'prefill us':>30s} {'ragged us':>30s} {'dense us':>28s} {'x ragged':>8s} {'beyond spread':>13s} "
             f"{'x dense':>7s} {'TFLOP/s':>8s} {'max |diff|':>10s}"]
    print("\n".join(lines), flush=True)
    torch.manual_seed(0)
    fmt = lambda t: f"{t[0]:9.1f} ({t[1]:.1f} ... {t[2]:.1f})"
    with torch.no_grad():
        for name, H, Hk, D, counts, cached, causal in ROWS:
            if a.only not in name:
                continue
            new, old, dense, copies, diff = case(H, Hk, D, counts, cached, causal, torch.float16 if name.startswith("f16") else DT)
            if a.calls > 0:
                for _ in range(a.calls):
                    new()
                torch.cuda.synchronize()
                continue
            fns = [new, old] + ([dense] if dense is not None else [])
            # long rows take fewer steps: a row's timing stays around a second per route and round at most
            pairs = visible_pairs(counts, cached, causal)
            steps = max(3, min(a.steps, int(2e10 / max(pairs * H * D, 1))))
            res = ab(fns, a.rounds, steps)
            t_n, t_o = res[0], res[1]
            t_d = res[2] if dense is not None else None
            spread = max(t_n[2] - t_n[1], t_o[2] - t_o[1])
            verdict = ("faster" if t_o[0] > t_n[0] else "slower") + (", yes" if abs(t_o[0] - t_n[0]) > spread else ", within")
            lines.append(f"{name:28s} {copies:6d} {pairs / 1e6:8.2f} {fmt(t_n):>30s} {fmt(t_o):>30s} {(fmt(t_d) if t_d else '-'):>28s} {t_o[0] / t_n[0]:7.2f}x "
                         f"{verdict:>13s} {(f'{t_d[0] / t_n[0]:.2f}x' if t_d else '-'):>7s} {4.0 * D * H * pairs / t_n[0] / 1e6:8.1f} {diff:10.2e}")
            print(lines[-1], flush=True)
            del new, old, dense, fns
            torch.cuda.empty_cache()
    if a.calls > 0:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
