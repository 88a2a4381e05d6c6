#!/usr/bin/env python3
"""Decoding against a key/value cache: flash_cosine_sim_attention_with_kvcache against the best the dense API can do on the same data, in
ONE process, the calls alternated round by round (bf16, causal, scale 8; median over the rounds of the per-call time of `--steps`
back-to-back calls, HIP events).

  dense baseline, equal lengths: flash_cosine_sim_attention(q, k_cache[:, :, :L], v_cache[:, :, :L], causal=True) (sliced views, no copy)
  dense baseline, ragged lengths (N = 1): the dense call over the whole capacity with a key mask (mask and causal cannot be combined;
                                          with N = 1 a causal row sees every cached key, so the masked call computes the same rows)
Reported per row: microseconds per call, effective GB/s = valid K + V bytes / time (the floor of a decode step is reading them once),
its share of the ~6.3 TB/s a copy reaches, and the speed-up over the dense call.  Targets: faster than dense on every row; >= 60 % of
the copy rate where the valid K + V bytes exceed 256 MB; a ragged batch within 1.2x of an equal-length batch with the same sum of L_b.
usage: decode_ab.py [--rounds R] [--steps K] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flash_cosine_sim_attention_amd as F  # noqa: E402

DT = torch.bfloat16
COPY_GBS = 6300.0

# (label, B, H, Hk, L (or per-sequence list), D)
SHAPES = [
    ("B1 H32 Hk8 L8k D128", 1, 32, 8, 8192, 128),
    ("B1 H32 Hk8 L32k D128", 1, 32, 8, 32768, 128),
    ("B1 H32 Hk8 L128k D128", 1, 32, 8, 131072, 128),
    ("B8 H32 Hk8 L4k D128", 8, 32, 8, 4096, 128),
    ("B8 H32 Hk8 L32k D128", 8, 32, 8, 32768, 128),
    ("B32 H32 Hk8 L2k D128", 32, 32, 8, 2048, 128),
    ("B16 H8 Hk8 L8k D64", 16, 8, 8, 8192, 64),
]
RAGGED = [1024, 30720, 2048, 16384, 512, 8192, 4096, 2560]      # sum 65536 = 8 x 8192


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
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            times[i].append(timed(f, steps))
    return [statistics.median(t) for t in times]


def case(B, H, Hk, lens, D, N, ragged):
    cap = max(lens)
    q = torch.randn(B, H, N, D, device="cuda", dtype=DT)
    kc, vc = (torch.randn(B, Hk, cap, D, device="cuda", dtype=DT) for _ in range(2))
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    new = lambda: F.flash_cosine_sim_attention_with_kvcache(q, kc, vc, cache_seqlens=sl, max_seqlen_k=cap, causal=True)
    if ragged:
        mask = torch.arange(cap, device="cuda")[None, :] < sl[:, None].long()
        dense = lambda: F.flash_cosine_sim_attention(q, kc, vc, mask=mask)
    else:
        L = lens[0]
        ks, vs = kc[:, :, :L], vc[:, :, :L]
        dense = lambda: F.flash_cosine_sim_attention(q, ks, vs, causal=True)
    valid = sum(lens) * Hk * D * 2 * 2
    return new, dense, valid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_ab.txt"))
    a = ap.parse_args()
    lines = [f"# tools/decode_ab.py --rounds {a.rounds} --steps {a.steps}: bf16, causal, scale 8; median us per call; "
             f"GB/s = valid K+V bytes / time; copy rate {COPY_GBS:.0f} GB/s",
             f"{'shape':34s} {'N':>2s} {'valid MB':>9s} {'new us':>9s} {'dense us':>9s} {'speed-up':>8s} {'new GB/s':>9s} {'% copy':>7s}"]
    rows = []
    torch.manual_seed(0)
    with torch.no_grad():
        for label, B, H, Hk, L, D in SHAPES + [("ragged B8 H32 Hk8 sum 64k D128", 8, 32, 8, RAGGED, 128)]:
            for N in (1, 4):
                ragged = isinstance(L, list)
                if ragged and N != 1:
                    continue
                lens = L if ragged else [L] * B
                new, dense, valid = case(B, H, Hk, lens, D, N, ragged)
                t_new, t_dense = ab([new, dense], a.rounds, a.steps)
                gbs = valid / t_new / 1e3
                rows.append((label, N, valid, t_new, t_dense))
                lines.append(f"{label:34s} {N:2d} {valid / 1e6:9.1f} {t_new:9.1f} {t_dense:9.1f} {t_dense / t_new:7.2f}x {gbs:9.0f} "
                             f"{100 * gbs / COPY_GBS:6.1f}%")
                print(lines[-1], flush=True)
                del new, dense
                torch.cuda.empty_cache()
    faster = all(r[4] > r[3] for r in rows)
    big = [r for r in rows if r[2] > 256e6]
    bw = all(r[2] / r[3] / 1e3 >= 0.6 * COPY_GBS for r in big)
    # the equal-length batch with the same sum of L_b (8 x 8192), same process
    with torch.no_grad():
        new_eq, _, _ = case(8, 32, 8, [8192] * 8, 128, 1, False)
        new_rag, _, _ = case(8, 32, 8, RAGGED, 128, 1, True)
        t_eq, t_rag = ab([new_eq, new_rag], a.rounds, a.steps)
    lines.append(f"ragged batch (sum L_b 65536): {t_rag:.1f} us; equal lengths 8 x 8192: {t_eq:.1f} us; ratio {t_rag / t_eq:.2f}")
    lines.append(f"target faster than dense on every row: {'met' if faster else 'NOT met'}")
    lines.append(f"target >= 60 % of the copy rate where valid K+V > 256 MB ({len(big)} rows): {'met' if bw else 'NOT met'}")
    lines.append(f"target ragged within 1.2x of equal lengths: {'met' if t_rag <= 1.2 * t_eq else 'NOT met'}")
    for ln in lines[-4:]:
        print(ln)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
