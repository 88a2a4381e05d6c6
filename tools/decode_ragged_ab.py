#!/usr/bin/env python3
"""Ragged decode steps: flash_cosine_sim_attention_varlen_with_kvcache against what the package offered before it, in ONE process, the
calls alternated round by round and warm (bf16, causal, scale 8, H 32, Hk 8, D 128 unless the shape says otherwise; per-call time of
`--steps` back-to-back calls between HIP events; median, with the min ... max over the rounds as the run-to-run spread).

  (a) mixed batches: B = 32 and 64 sequences with caches of 2k ... 32k positions; N_b mostly 1, a few 4-token sequences and one 256-token
      chunk; every token appends its key and value.  The alternative is the loop of per-sequence flash_cosine_sim_attention_with_kvcache
      calls (three launches each), on its own copy of the caches.
  (b) equal-N batches (N = 1 and 4) on the shapes of profiles/decode_ab.txt, no append: the ragged call (cu_seqlens_q = N * arange)
      against the existing batched call.  The same kernel body runs; the difference is the tile lookup (a binary search over the table per
      workgroup), the B idle slots of the grid and the packed output indexing.
No threshold is asserted: the file records what was measured.
usage: decode_ragged_ab.py [--rounds R] [--steps K] [--out FILE] [--only a|b]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flash_cosine_sim_attention_amd as F  # noqa: E402

DT = torch.bfloat16
H, HK, D = 32, 8, 128

# (a): (label, B, longest cache)
MIXED = [("B32 caches<=2k", 32, 2048), ("B32 caches<=8k", 32, 8192), ("B32 caches<=32k", 32, 32768),
         ("B64 caches<=2k", 64, 2048), ("B64 caches<=8k", 64, 8192), ("B64 caches<=32k", 64, 32768)]
# (b): the shapes of tools/decode_ab.py (label, B, H, Hk, L, D)
EQUAL = [("B1 H32 Hk8 L8k D128", 1, 32, 8, 8192, 128), ("B1 H32 Hk8 L32k D128", 1, 32, 8, 32768, 128),
         ("B1 H32 Hk8 L128k D128", 1, 32, 8, 131072, 128), ("B8 H32 Hk8 L4k D128", 8, 32, 8, 4096, 128),
         ("B8 H32 Hk8 L32k D128", 8, 32, 8, 32768, 128), ("B32 H32 Hk8 L2k D128", 32, 32, 8, 2048, 128),
         ("B16 H8 Hk8 L8k D64", 16, 8, 8, 8192, 64)]


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


def mixed_case(B, longest, gen):
    """N_b: one 256-token chunk, three 4-token sequences, the rest plain decodes; cached lengths uniform in [longest / 2, longest - N_b]"""
    counts = [1] * B
    counts[B // 2] = 256
    for b in (1, B // 3, B - 2):
        counts[b] = 4
    cached = [int(torch.randint(longest // 2, longest - n + 1, (1,), generator=gen)) for n in counts]
    total = sum(counts)
    q = torch.randn(total, H, D, device="cuda", dtype=DT)
    kn, vn = (torch.randn(total, HK, D, device="cuda", dtype=DT) for _ in range(2))
    kc, vc = (torch.randn(B, HK, longest, D, device="cuda", dtype=DT) for _ in range(2))
    kc2, vc2 = kc.clone(), vc.clone()
    cu = torch.tensor([0] + torch.tensor(counts).cumsum(0).tolist(), dtype=torch.int32, device="cuda")
    sl = torch.tensor(cached, dtype=torch.int32, device="cuda")
    max_q, max_k = max(counts), max(c + n for c, n in zip(cached, counts))
    ragged = lambda: F.flash_cosine_sim_attention_varlen_with_kvcache(q, kc, vc, cu, kn, vn, sl, max_seqlen_q=max_q, max_seqlen_k=max_k,
                                                                     causal=True)
    c = cu.tolist()
    rows = lambda t, b: t[c[b]:c[b + 1]].permute(1, 0, 2).unsqueeze(0)
    per = [(rows(q, b), kc2[b:b + 1], vc2[b:b + 1], rows(kn, b), rows(vn, b), sl[b:b + 1], cached[b] + counts[b]) for b in range(B)]

    def loop():
        for qb, kb, vb, knb, vnb, slb, mk in per:
            F.flash_cosine_sim_attention_with_kvcache(qb, kb, vb, knb, vnb, slb, max_seqlen_k=mk, causal=True)

    valid = sum(c_ + n for c_, n in zip(cached, counts)) * HK * D * 2 * 2
    return ragged, loop, total, valid


def equal_case(B, h, hk, L, d, N):
    q4 = torch.randn(B, h, N, d, device="cuda", dtype=DT)
    q3 = q4.permute(0, 2, 1, 3).reshape(B * N, h, d).contiguous()
    kc, vc = (torch.randn(B, hk, L, d, device="cuda", dtype=DT) for _ in range(2))
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda") * N
    batched = lambda: F.flash_cosine_sim_attention_with_kvcache(q4, kc, vc, cache_seqlens=sl, max_seqlen_k=L, causal=True)
    ragged = lambda: F.flash_cosine_sim_attention_varlen_with_kvcache(q3, kc, vc, cu, cache_seqlens=sl, max_seqlen_q=N, max_seqlen_k=L,
                                                                     causal=True)
    return ragged, batched


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", choices=("a", "b"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_ragged_ab.txt"))
    a = ap.parse_args()
    lines = [f"# tools/decode_ragged_ab.py --rounds {a.rounds} --steps {a.steps}: bf16, causal, scale 8; us per call: median (min ... max over the rounds)"]
    gen = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    fmt = lambda t: f"{t[0]:9.1f} ({t[1]:.1f} ... {t[2]:.1f})"
    with torch.no_grad():
        if a.only != "b":
            lines.append("# (a) mixed batches, H32 Hk8 D128, append: one 256-token chunk, three 4-token sequences, the rest 1 token; "
                         "ragged call vs the loop of per-sequence calls")
            lines.append(f"{'batch':18s} {'tokens':>6s} {'valid MB':>9s} {'ragged us':>32s} {'per-sequence loop us':>36s} {'speed-up':>9s}")
            for label, B, longest in MIXED:
                ragged, loop, total, valid = mixed_case(B, longest, gen)
                t_r, t_l = ab([ragged, loop], a.rounds, max(a.steps // 4, 3))
                lines.append(f"{label:18s} {total:6d} {valid / 1e6:9.1f} {fmt(t_r):>32s} {fmt(t_l):>36s} {t_l[0] / t_r[0]:8.2f}x")
                print(lines[-1], flush=True)
                del ragged, loop
                torch.cuda.empty_cache()
        if a.only != "a":
            lines.append("# (b) equal-N batches, no append: ragged call vs the existing batched call (same kernel body); "
                         "ratio = ragged / batched, lookup = ragged - batched")
            lines.append(f"{'shape':24s} {'N':>2s} {'ragged us':>32s} {'batched us':>32s} {'ratio':>6s} {'lookup us':>9s} {'batched spread':>14s}")
            for label, B, h, hk, L, d in EQUAL:
                for N in (1, 4):
                    ragged, batched = equal_case(B, h, hk, L, d, N)
                    t_r, t_b = ab([ragged, batched], a.rounds, a.steps)
                    lines.append(f"{label:24s} {N:2d} {fmt(t_r):>32s} {fmt(t_b):>32s} {t_r[0] / t_b[0]:6.3f} {t_r[0] - t_b[0]:9.1f} "
                                 f"{100 * (t_b[2] - t_b[1]) / t_b[0]:13.1f}%")
                    print(lines[-1], flush=True)
                    del ragged, batched
                    torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
