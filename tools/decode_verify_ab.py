#!/usr/bin/env python3
"""The 64-row verify kernel of 16-bit and fp8 caches: flash_cosine_sim_attention_verify_with_kvcache against the calls that served the same
arguments before it.  The protocol is tools/decode_tree_ab.py's: ONE process, the routes alternated round by round and warm (bf16, scale 8,
H 32, Hk 8, D 128, paged caches with pages of 16, every token appends its key and value; per-call time of `--steps` back-to-back calls
between HIP events; median, with the min ... max over the rounds as the run-to-run spread).  Every route rotates over enough copies of the
cache pool that at least ROTATE_BYTES of keys and values pass before a buffer comes round again -- more than the 256 MB last-level cache --
so the figures are those of caches coming from HBM, as in a serving step.

Verify rows (B sequences of N_b step tokens each against caches of L positions after the step), on a bf16 and on an fp8 (e4m3fn) cache:
  chain / tree        the new call with the chain mask (word i = bits 0 .. i) / a random tree (the parent of token t uniform in [0, t))
  old chain / tree    flash_cosine_sim_attention_tree_with_kvcache on the same arguments: the one-wave decode kernel with the mask
Prefill rows (B sequences of N_b prompt tokens on `cached` positions, tree_mask=None, causal=True, bf16 cache):
  new                 the new call
  ragged / prefill    flash_cosine_sim_attention_varlen_with_kvcache / flash_cosine_sim_attention_prefill_with_kvcache
Ratios are of the medians (below 1: the new call is faster).  "verdict" applies the rule the README uses: a row counts as faster or slower
only where the medians differ by more than the sum of both routes' spreads (max - min); otherwise "same".  No threshold is asserted.
usage: decode_verify_ab.py [--rounds R] [--steps K] [--out FILE]"""
import argparse
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import flash_cosine_sim_attention_amd as F  # noqa: E402
from decode_tree_ab import ab, chain_words, rotating, tree_words  # noqa: E402

DT, E4M3 = torch.bfloat16, torch.float8_e4m3fn
H, HK, D, PAGE = 32, 8, 128, 16
VERIFY = [(B, N, L) for L in (4096, 32768) for B in (8, 64) for N in (8, 32, 64)]
PREFILL = [(B, N, cached) for cached in (8192, 32768) for B in (1, 8) for N in (64, 256)]
ROTATE_BYTES = 600e6


def pools_of(blocks, nbytes, fp8):
    """copies of a (K, V) pool of `blocks` pages: normal bf16 values, or finite e4m3fn codes of either sign (magnitudes up to 240)"""
    def one():
        if fp8:
            return (torch.randint(0, 120, (blocks, HK, PAGE, D), device="cuda", dtype=torch.uint8)
                    | (torch.randint(0, 2, (blocks, HK, PAGE, D), device="cuda", dtype=torch.uint8) << 7)).view(E4M3)
        return torch.empty(blocks, HK, PAGE, D, device="cuda", dtype=DT).normal_()
    return [(one(), one()) for _ in range(max(1, -(-int(ROTATE_BYTES) // nbytes)))]


def case(B, N, L, fp8):
    """the packed step of B x N tokens whose caches hold L positions after it: (q, cu, kn, vn, sl), the pools, the keywords"""
    pages = -(-L // PAGE)
    nbytes = B * pages * PAGE * HK * D * 2 * (1 if fp8 else 2)
    q = torch.randn(B * N, H, D, device="cuda", dtype=DT)
    kn, vn = (torch.randn(B * N, HK, D, device="cuda", dtype=DT) for _ in range(2))
    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda") * N
    sl = torch.full((B,), L - N, dtype=torch.int32, device="cuda")
    kw = dict(block_table=torch.randperm(B * pages, device="cuda").to(torch.int32).view(B, pages), max_seqlen_q=N, max_seqlen_k=pages * PAGE)
    if fp8:
        kw.update(k_scale=torch.rand(B, HK, device="cuda") * 0.02 + 0.01, v_scale=torch.rand(B, HK, device="cuda") * 0.02 + 0.01)
    return (q, cu, kn, vn, sl), pools_of(B * pages, nbytes, fp8), kw, nbytes


def route(fn, args, pools, kw, **how):
    q, cu, kn, vn, sl = args
    return rotating([lambda k=k, v=v: fn(q, k, v, cu, kn, vn, sl, **kw, **how) for k, v in pools])


def verdict(new, old):
    if abs(new[0] - old[0]) <= (new[2] - new[1]) + (old[2] - old[1]):
        return "same"
    return "faster" if new[0] < old[0] else "SLOWER"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_verify_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_verify_ab.py measures on the GPU: no GPU visible")
    new, old = F.flash_cosine_sim_attention_verify_with_kvcache, F.flash_cosine_sim_attention_tree_with_kvcache
    ragged, prefill = F.flash_cosine_sim_attention_varlen_with_kvcache, F.flash_cosine_sim_attention_prefill_with_kvcache
    lines = [f"# tools/decode_verify_ab.py --rounds {a.rounds} --steps {a.steps}: bf16 queries, scale 8, H{H} Hk{HK} D{D}, pages of {PAGE}, append; us per call: "
             "median (min ... max over the rounds); every route rotates over copies of the cache pool "
             f"(>= {ROTATE_BYTES / 1e6:.0f} MB between two uses of a buffer: HBM-resident, not cache-warm)",
             f"# device: {torch.cuda.get_device_name(0)}",
             f"{'verify step':24s} {'KV MB':>7s} {'copies':>6s} {'chain us':>28s} {'tree us':>28s} {'old chain us':>31s} {'old tree us':>31s} "
             f"{'chain/old':>9s} {'tree/old':>9s} {'verdict':>7s} {'|new-old|':>9s}"]
    torch.manual_seed(0)
    rng = random.Random(0)
    fmt = lambda t: f"{t[0]:9.1f} ({t[1]:.1f} ... {t[2]:.1f})"
    with torch.no_grad():
        for fp8 in (False, True):
            for B, N, L in VERIFY:
                args, pools, kw, nbytes = case(B, N, L, fp8)
                chain, tree = chain_words(B, N), tree_words(B, N, rng)
                routes = [route(new, args, pools, kw, tree_mask=chain), route(new, args, pools, kw, tree_mask=tree),
                          route(old, args, pools, kw, tree_mask=chain), route(old, args, pools, kw, tree_mask=tree)]
                diff = (routes[1]().float() - routes[3]().float()).abs().max().item()      # (different split counts: rounding only)
                t = ab(routes, a.rounds, a.steps)
                label = f"{'fp8' if fp8 else 'bf16'} B{B} N{N} L{L}"
                lines.append(f"{label:24s} {nbytes / 1e6:7.1f} {len(pools):6d} {fmt(t[0]):>28s} {fmt(t[1]):>28s} "
                             f"{fmt(t[2]):>31s} {fmt(t[3]):>31s} {t[0][0] / t[2][0]:8.3f}x {t[1][0] / t[3][0]:8.3f}x {verdict(t[1], t[3]):>7s} {diff:9.2e}")
                print(lines[-1], flush=True)
                del routes, pools
                torch.cuda.empty_cache()
        lines.append(f"{'prefill (causal)':24s} {'KV MB':>7s} {'copies':>6s} {'new us':>28s} {'ragged us':>28s} {'prefill us':>31s} {'new/ragged':>10s} "
                     f"{'verdict':>7s} {'new/prefill':>11s} {'verdict':>7s} {'|new-ragged|':>12s}")
        for B, N, cached in PREFILL:
            args, pools, kw, nbytes = case(B, N, cached + N, False)
            routes = [route(new, args, pools, kw, causal=True), route(ragged, args, pools, kw, causal=True), route(prefill, args, pools, kw, causal=True)]
            diff = (routes[0]().float() - routes[1]().float()).abs().max().item()
            t = ab(routes, a.rounds, a.steps)
            label = f"bf16 B{B} N{N} on {cached}"
            lines.append(f"{label:24s} {nbytes / 1e6:7.1f} {len(pools):6d} {fmt(t[0]):>28s} {fmt(t[1]):>28s} {fmt(t[2]):>31s} "
                         f"{t[0][0] / t[1][0]:9.3f}x {verdict(t[0], t[1]):>7s} {t[0][0] / t[2][0]:10.3f}x {verdict(t[0], t[2]):>7s} {diff:12.2e}")
            print(lines[-1], flush=True)
            del routes, pools
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
