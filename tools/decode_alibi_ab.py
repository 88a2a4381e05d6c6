#!/usr/bin/env python3
"""The linear position bias of the cached calls: flash_cosine_sim_attention_alibi_with_kvcache with the standard slopes 2^(-8 (h + 1) / H)
against flash_cosine_sim_attention_step_with_kvcache on identical arguments (the existing engine step, untouched by the bias work: the
reference for the time).  The protocol and the decode shapes are those of tools/decode_tree_ab.py: ONE process, the calls alternated round
by round and warm (bf16, H 32, Hk 8, D 128, paged caches with pages of 16, causal, every token appends its key and value; per-call time of
`--steps` back-to-back calls between HIP events; median, with the min ... max over the rounds as the run-to-run spread), every route
rotating over enough copies of the cache pool that at least ROTATE_BYTES of keys and values pass before a buffer comes round again.  One
more row is a 1024-token prompt chunk (one sequence: the chunk kernel).

Per row:
  step      the step call at scale 8: the static exponent regime
  step dyn  the step call at scale 80 (bf16: scale * groups above 75, the static regime's limit): the per-row-shift regime without a bias --
            what the regime alone costs on the same shape
  alibi     the position-bias call at scale 8 (always the per-row-shift regime)
"dyn/step" and "alibi/step" are ratios of medians; "step spread" the (max - min) / median of the step timings, the yardstick for them.
No threshold is asserted: the file records what was measured.
usage: decode_alibi_ab.py [--rounds R] [--steps K] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flash_cosine_sim_attention_amd as F  # noqa: E402

DT = torch.bfloat16
H, HK, D, PAGE = 32, 8, 128, 16
SHAPES = [(B, N, L) for L in (4096, 32768) for B in (8, 64) for N in (8, 32, 64)] + [(1, 1024, 4096)]
ROTATE_BYTES = 600e6
step_call = F.flash_cosine_sim_attention_step_with_kvcache
alibi_call = F.flash_cosine_sim_attention_alibi_with_kvcache


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


def case(B, N, L):
    pages = L // PAGE
    kv_bytes = B * L * HK * D * 2 * 2
    copies = max(1, -(-int(ROTATE_BYTES) // kv_bytes))
    q = torch.randn(B * N, H, D, device="cuda", dtype=DT)
    kn, vn = (torch.randn(B * N, HK, D, device="cuda", dtype=DT) for _ in range(2))
    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda") * N
    sl = torch.full((B,), L - N, dtype=torch.int32, device="cuda")
    table = torch.randperm(B * pages, device="cuda").to(torch.int32).view(B, pages)
    pools = [tuple(torch.empty(B * pages, HK, PAGE, D, device="cuda", dtype=DT).normal_() for _ in range(2)) for _ in range(copies)]
    slopes = torch.tensor([2.0 ** (-8.0 * (h + 1) / H) for h in range(H)], dtype=torch.float32, device="cuda")
    kw = dict(block_table=table, max_seqlen_q=N, max_seqlen_k=L, causal=True, max_decode_tokens=B * N)

    def route(fn, **how):
        return rotating([lambda k=k, v=v: fn(q, k, v, cu, kn, vn, sl, **kw, **how) for k, v in pools])

    return route(step_call, scale=8), route(step_call, scale=80), route(alibi_call, scale=8, alibi_slopes=slopes), copies, kv_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_alibi_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_alibi_ab.py measures on the GPU: no GPU visible")
    lines = [f"# tools/decode_alibi_ab.py --rounds {a.rounds} --steps {a.steps}: bf16, H{H} Hk{HK} D{D}, pages of {PAGE}, causal, append; us per call: "
             "median (min ... max over the rounds); the routes rotate over `copies` cache pools "
             f"(>= {ROTATE_BYTES / 1e6:.0f} MB of keys and values between two uses of a buffer: HBM-resident, not cache-warm)",
             f"# device: {torch.cuda.get_device_name(0)}",
             f"{'shape':18s} {'KV MB':>8s} {'copies':>6s} {'step us':>30s} {'step dyn us':>30s} {'alibi us':>30s} {'dyn/step':>9s} {'alibi/step':>10s} "
             f"{'alibi/dyn':>9s} {'step spread':>11s}"]
    torch.manual_seed(0)
    fmt = lambda t: f"{t[0]:9.1f} ({t[1]:.1f} ... {t[2]:.1f})"
    with torch.no_grad():
        for B, N, L in SHAPES:
            step, dyn, alibi, copies, kv_bytes = case(B, N, L)
            t_step, t_dyn, t_alibi = ab([step, dyn, alibi], a.rounds, a.steps)
            lines.append(f"{f'B{B} N{N} L{L}':18s} {kv_bytes / 1e6:8.1f} {copies:6d} {fmt(t_step):>30s} {fmt(t_dyn):>30s} {fmt(t_alibi):>30s} "
                         f"{t_dyn[0] / t_step[0]:8.3f}x {t_alibi[0] / t_step[0]:9.3f}x {t_alibi[0] / t_dyn[0]:8.3f}x "
                         f"{100 * (t_step[2] - t_step[1]) / t_step[0]:10.1f}%")
            print(lines[-1], flush=True)
            del step, dyn, alibi
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
