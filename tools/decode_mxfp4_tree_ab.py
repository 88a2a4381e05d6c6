#!/usr/bin/env python3
"""Tree attention against MXFP4 caches: flash_cosine_sim_attention_mxfp4_tree_with_kvcache (the 64-row verify kernel with key splits) against
the two routes a speculative decoder had before it, on identical arguments.  The protocol is tools/decode_tree_ab.py's: ONE process, the
routes alternated round by round and warm (bf16, scale 8, H 32, Hk 8, D 128, paged caches with pages of 16, every token appends its key and
value; per-call time of `--steps` back-to-back calls between HIP events; median, with the min ... max over the rounds as the run-to-run
spread).  Every route rotates over enough copies of its cache pool that at least ROTATE_BYTES of codes and scales (of 16-bit keys and
values) pass before a buffer comes round again -- more than the 256 MB last-level cache -- so the figures are those of caches coming from
HBM, as in a serving step.

Per row (B sequences of N_b step tokens each against caches of L positions after the step):
  chain    the new call with the chain mask (word i = bits 0 .. i): computes what causal computes
  tree     the new call with a random tree (the parent of token t uniform in [0, t); word = ancestors and self)
  causal   flash_cosine_sim_attention_mxfp4_with_kvcache, ragged, causal=True: the same work under the wrong mask, the only MXFP4 route before
  bf16     flash_cosine_sim_attention_tree_with_kvcache with the random tree on the DEQUANTISED caches (16-bit: 3.76x the bytes)
"chain/causal" and "tree/bf16" are ratios of the medians (below 1: the new call is faster); "causal spread" is the (max - min) / median of
the causal timings, the yardstick for them.  No threshold is asserted: the file records what was measured.
usage: decode_mxfp4_tree_ab.py [--rounds R] [--steps K] [--out FILE]"""
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

DT = torch.bfloat16
H, HK, D, PAGE = 32, 8, 128, 16
SHAPES = [(B, N, L) for L in (4096, 32768) for B in (8, 64) for N in (8, 32, 64)]
ROTATE_BYTES = 600e6


def mx_pool(blocks):
    """random codes and scale bytes (exponents -7 ... 2) of a pool of `blocks` pages: (k codes, v codes, k scales, v scales)"""
    codes = lambda: torch.randint(0, 256, (blocks, HK, PAGE, D // 2), device="cuda", dtype=torch.uint8)
    scales = lambda: torch.randint(120, 130, (blocks, HK, PAGE, D // 32), device="cuda", dtype=torch.uint8)
    return codes(), codes(), scales(), scales()


def dense_pool(mx, chunk=4096):
    """the 16-bit caches holding the pool's values, dequantised a few thousand pages at a time"""
    out = [torch.empty(*mx[0].shape[:3], D, device="cuda", dtype=DT) for _ in range(2)]
    for at in range(0, mx[0].shape[0], chunk):
        for o, c, s in zip(out, mx[:2], mx[2:]):
            o[at:at + chunk] = F.mxfp4_dequantize(c[at:at + chunk], s[at:at + chunk], DT)
    return out


def case(B, N, L, rng):
    pages = L // PAGE
    mx_bytes, kv_bytes = B * L * HK * (D // 2 + D // 32) * 2, B * L * HK * D * 2 * 2
    q = torch.randn(B * N, H, D, device="cuda", dtype=DT)
    kn, vn = (torch.randn(B * N, HK, D, device="cuda", dtype=DT) for _ in range(2))
    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda") * N
    sl = torch.full((B,), L - N, dtype=torch.int32, device="cuda")
    table = torch.randperm(B * pages, device="cuda").to(torch.int32).view(B, pages)
    mx_pools = [mx_pool(B * pages) for _ in range(max(1, -(-int(ROTATE_BYTES) // mx_bytes)))]
    dense_pools = [dense_pool(mx_pools[i % len(mx_pools)]) for i in range(max(1, -(-int(ROTATE_BYTES) // kv_bytes)))]
    chain, tree = chain_words(B, N), tree_words(B, N, rng)
    kw = dict(block_table=table, max_seqlen_q=N, max_seqlen_k=L)
    new = lambda words: rotating([lambda p=p: F.flash_cosine_sim_attention_mxfp4_tree_with_kvcache(q, *p, cu, kn, vn, sl, tree_mask=words, **kw)
                                  for p in mx_pools])
    causal = rotating([lambda p=p: F.flash_cosine_sim_attention_mxfp4_with_kvcache(q, *p, cu, kn, vn, sl, causal=True, **kw) for p in mx_pools])
    bf16 = rotating([lambda p=p: F.flash_cosine_sim_attention_tree_with_kvcache(q, *p, cu, kn, vn, sl, tree_mask=tree, **kw) for p in dense_pools])
    # what the routes disagree by on the first pool: the new call against the 16-bit tree call (the append quantises only on the MXFP4 side,
    # so the step's own keys differ by the quantisation), and its chain mask against the MXFP4 causal call (the same values: rounding only)
    d_tree = (new(tree)().float() - bf16().float()).abs().max().item()
    d_chain = (new(chain)().float() - causal().float()).abs().max().item()
    return (new(chain), new(tree), causal, bf16), (len(mx_pools), len(dense_pools)), (mx_bytes, kv_bytes), (d_chain, d_tree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_mxfp4_tree_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_mxfp4_tree_ab.py measures on the GPU: no GPU visible")
    lines = [f"# tools/decode_mxfp4_tree_ab.py --rounds {a.rounds} --steps {a.steps}: bf16, scale 8, H{H} Hk{HK} D{D}, pages of {PAGE}, append; us per call: "
             "median (min ... max over the rounds); every route rotates over copies of its cache pool "
             f"(>= {ROTATE_BYTES / 1e6:.0f} MB between two uses of a buffer: HBM-resident, not cache-warm); copies: MXFP4 / 16-bit",
             f"# device: {torch.cuda.get_device_name(0)}",
             f"{'shape':16s} {'MX MB':>7s} {'KV MB':>7s} {'copies':>7s} {'chain us':>30s} {'tree us':>30s} {'causal us':>30s} {'bf16 tree us':>30s} "
             f"{'chain/causal':>12s} {'causal spread':>13s} {'tree/bf16':>9s} {'|chain-causal|':>14s} {'|tree-bf16|':>11s}"]
    torch.manual_seed(0)
    rng = random.Random(0)
    fmt = lambda t: f"{t[0]:9.1f} ({t[1]:.1f} ... {t[2]:.1f})"
    with torch.no_grad():
        for B, N, L in SHAPES:
            routes, copies, nbytes, diff = case(B, N, L, rng)
            t_chain, t_tree, t_causal, t_bf16 = ab(list(routes), a.rounds, a.steps)
            lines.append(f"{f'B{B} N{N} L{L}':16s} {nbytes[0] / 1e6:7.1f} {nbytes[1] / 1e6:7.1f} {f'{copies[0]}/{copies[1]}':>7s} {fmt(t_chain):>30s} "
                         f"{fmt(t_tree):>30s} {fmt(t_causal):>30s} {fmt(t_bf16):>30s} {t_chain[0] / t_causal[0]:11.3f}x "
                         f"{100 * (t_causal[2] - t_causal[1]) / t_causal[0]:12.1f}% {t_tree[0] / t_bf16[0]:8.3f}x {diff[0]:14.2e} {diff[1]:11.2e}")
            print(lines[-1], flush=True)
            del routes
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
