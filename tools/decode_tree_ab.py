#!/usr/bin/env python3
"""Tree attention for speculative decoding: flash_cosine_sim_attention_tree_with_kvcache with tree_mask against
flash_cosine_sim_attention_varlen_with_kvcache with causal=True on identical arguments (the existing ragged call, untouched by the tree
work: the reference for the time), and
kvcache_keep_accepted against the same bytes moved with torch.  ONE process, the calls alternated round by round and warm (bf16, scale
8, H 32, Hk 8, D 128, paged caches with pages of 16, every token appends its key and value; per-call time of `--steps` back-to-back calls
between HIP events; median, with the min ... max over the rounds as the run-to-run spread).  Every decode route rotates over enough copies
of the cache pool that at least ROTATE_BYTES of keys and values pass before a buffer comes round again (more than the 256 MB last-level
cache), so the figures are those of caches coming from HBM, as in a serving step; "copies" says how many.

Per row (B sequences of N_b step tokens each against caches of L positions after the step):
  chain    the tree call with the chain mask (word i = bits 0 .. i): computes exactly what causal computes, bit for bit
  causal   the existing ragged call with causal=True
  tree     the tree call with a random tree (the parent of token t uniform in [0, t); word = ancestors and self)
  keep     kvcache_keep_accepted accepting 4 of the N_b tokens (0, N_b / 4, N_b / 2, N_b - 1) on the paged pool
  torch    the same rows moved with torch.index_select + index_copy_ on a CONTIGUOUS cache [B, Hk, 4096, D] (uniform cache_seqlens, so one
           index vector serves the batch; two calls each for K and V)
"chain/causal" is the ratio of the medians; "causal spread" the (max - min) / median of the causal timings, the yardstick for it.
No threshold is asserted: the file records what was measured.
usage: decode_tree_ab.py [--rounds R] [--steps K] [--out FILE]"""
import argparse
import os
import random
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flash_cosine_sim_attention_amd as F  # noqa: E402

DT = torch.bfloat16
H, HK, D, PAGE = 32, 8, 128, 16
SHAPES = [(B, N, L) for L in (4096, 32768) for B in (8, 64) for N in (8, 32, 64)]
ROTATE_BYTES = 600e6
ragged = F.flash_cosine_sim_attention_varlen_with_kvcache
tree_call = F.flash_cosine_sim_attention_tree_with_kvcache


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


def signed(words):
    return torch.tensor([w - (1 << 64) if w >= 1 << 63 else w for w in words], dtype=torch.int64, device="cuda")


def chain_words(B, N):
    return signed([(1 << (i + 1)) - 1 for i in range(N)] * B)


def tree_words(B, N, rng):
    out = []
    for _ in range(B):
        own = []
        for t in range(N):
            own.append((1 << t) | (own[rng.randrange(t)] if t else 0))
        out += own
    return signed(out)


def case(B, N, L, rng):
    pages = L // PAGE
    kv_bytes = B * L * HK * D * 2 * 2
    copies = max(1, -(-int(ROTATE_BYTES) // kv_bytes))
    q = torch.randn(B * N, H, D, device="cuda", dtype=DT)
    kn, vn = (torch.randn(B * N, HK, D, device="cuda", dtype=DT) for _ in range(2))
    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda") * N
    sl = torch.full((B,), L - N, dtype=torch.int32, device="cuda")
    table = torch.randperm(B * pages, device="cuda").to(torch.int32).view(B, pages)
    pools = [tuple(torch.empty(B * pages, HK, PAGE, D, device="cuda", dtype=DT).normal_() for _ in range(2)) for _ in range(copies)]
    chain, tree = chain_words(B, N), tree_words(B, N, rng)
    kw = dict(block_table=table, max_seqlen_q=N, max_seqlen_k=L)

    def route(**how):
        fn = tree_call if "tree_mask" in how else ragged
        return rotating([lambda k=k, v=v: fn(q, k, v, cu, kn, vn, sl, **kw, **how) for k, v in pools])

    same = torch.equal(tree_call(q, *pools[0], cu, kn, vn, sl, tree_mask=chain, **kw), ragged(q, *pools[0], cu, kn, vn, sl, causal=True, **kw))
    accepted = torch.tensor([[0, N // 4, N // 2, N - 1]] * B, dtype=torch.int32, device="cuda")
    num = torch.full((B,), 4, dtype=torch.int32, device="cuda")
    keep = rotating([lambda k=k, v=v: F.kvcache_keep_accepted(k, v, sl, accepted, num, block_table=table) for k, v in pools])
    # the torch route: a contiguous cache, one index vector for the whole batch
    ck, cv = (torch.empty(B, HK, 4096, D, device="cuda", dtype=DT).normal_() for _ in range(2))
    start = 4096 - N
    src = (accepted[0].long() + start)
    dst = torch.arange(4, device="cuda") + start

    def by_torch():
        ck.index_copy_(2, dst, ck.index_select(2, src))
        cv.index_copy_(2, dst, cv.index_select(2, src))

    return route(tree_mask=chain), route(causal=True), route(tree_mask=tree), keep, by_torch, copies, kv_bytes, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_tree_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_tree_ab.py measures on the GPU: no GPU visible")
    lines = [f"# tools/decode_tree_ab.py --rounds {a.rounds} --steps {a.steps}: bf16, scale 8, H{H} Hk{HK} D{D}, pages of {PAGE}, append; us per call: "
             "median (min ... max over the rounds); the decode routes rotate over `copies` cache pools "
             f"(>= {ROTATE_BYTES / 1e6:.0f} MB of keys and values between two uses of a buffer: HBM-resident, not cache-warm)",
             f"# device: {torch.cuda.get_device_name(0)}",
             f"{'shape':16s} {'KV MB':>8s} {'copies':>6s} {'chain us':>30s} {'causal us':>30s} {'chain/causal':>12s} {'causal spread':>13s} {'tree us':>30s} "
             f"{'tree/causal':>11s} {'keep us':>24s} {'torch us':>24s} {'torch/keep':>10s} {'chain==causal':>13s}"]
    torch.manual_seed(0)
    rng = random.Random(0)
    fmt = lambda t: f"{t[0]:9.1f} ({t[1]:.1f} ... {t[2]:.1f})"
    with torch.no_grad():
        for B, N, L in SHAPES:
            chain, causal, tree, keep, by_torch, copies, kv_bytes, same = case(B, N, L, rng)
            t_chain, t_causal, t_tree = ab([chain, causal, tree], a.rounds, a.steps)
            t_keep, t_torch = ab([keep, by_torch], a.rounds, a.steps)
            lines.append(f"{f'B{B} N{N} L{L}':16s} {kv_bytes / 1e6:8.1f} {copies:6d} {fmt(t_chain):>30s} {fmt(t_causal):>30s} {t_chain[0] / t_causal[0]:11.3f}x "
                         f"{100 * (t_causal[2] - t_causal[1]) / t_causal[0]:12.1f}% {fmt(t_tree):>30s} {t_tree[0] / t_causal[0]:10.3f}x {fmt(t_keep):>24s} "
                         f"{fmt(t_torch):>24s} {t_torch[0] / t_keep[0]:9.2f}x {str(same):>13s}")
            print(lines[-1], flush=True)
            del chain, causal, tree, keep, by_torch
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
