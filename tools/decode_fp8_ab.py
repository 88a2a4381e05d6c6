#!/usr/bin/env python3
"""Decoding against an fp8 (e4m3fn) key/value cache against the 16-bit call on the same logical cache, in ONE process, the two calls
alternated round by round (bf16 queries, causal, scale 8, N = 1; per round the per-call time of `--steps` back-to-back calls, HIP events;
the median over the rounds is reported).  The shapes are those of tools/decode_ab.py.

  fp8   : flash_cosine_sim_attention_with_kvcache(q, k8, v8, k_scale=, v_scale=) -- codes of randn data under per-head power-of-two scales
  16-bit: the same call on bf16 caches holding scale * code exactly (the decode kernel as it was before fp8 caches existed)

Per row: both times, t16 / t8 (2x is the ceiling: the K + V bytes halve), the valid K + V bytes each call reads, each call's share of the
~6.3 TB/s a copy reaches, and the repeat-to-repeat spread: the larger of the two calls' (max - min) over the rounds.  Requirement: on no
row is the fp8 call slower than the 16-bit call by more than that row's spread.
usage: decode_fp8_ab.py [--rounds R] [--steps K] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flash_cosine_sim_attention_amd as F  # noqa: E402
from tools.decode_ab import COPY_GBS, RAGGED, SHAPES, timed  # noqa: E402

DT = torch.bfloat16
E4M3 = torch.float8_e4m3fn


def ab(fns, rounds, steps):
    """per-round times of every call, alternated"""
    for f in fns:                                  # warm-up
        f()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            times[i].append(timed(f, steps))
    return times


def caches(B, Hk, cap, D):
    """(codes, bf16 cache holding scale * code, scales [B, Hk]) of randn data; the scale is a power of two, so the bf16 cache is exact"""
    c8 = torch.empty(B, Hk, cap, D, device="cuda", dtype=torch.uint8).view(E4M3)
    c16 = torch.empty(B, Hk, cap, D, device="cuda", dtype=DT)
    s = torch.empty(B, Hk, device="cuda", dtype=torch.float32)
    for b in range(B):                             # per sequence: bounds the float32 temporaries
        x = torch.randn(Hk, cap, D, device="cuda", dtype=torch.float32)
        sb = torch.exp2(torch.ceil(torch.log2(x.abs().amax(dim=(1, 2)) / 448)))
        codes = (x / sb[:, None, None]).clamp(-448, 448).to(E4M3)
        c8.view(torch.uint8)[b], s[b] = codes.view(torch.uint8), sb
        c16[b] = (codes.float() * sb[:, None, None]).to(DT)
    return c8, c16, s


def case(B, H, Hk, lens, D, N):
    cap = max(lens)
    q = torch.randn(B, H, N, D, device="cuda", dtype=DT)
    k8, k16, ks = caches(B, Hk, cap, D)
    v8, v16, vs = caches(B, Hk, cap, D)
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    kv = F.flash_cosine_sim_attention_with_kvcache
    f8 = lambda: kv(q, k8, v8, cache_seqlens=sl, max_seqlen_k=cap, causal=True, k_scale=ks, v_scale=vs)
    f16 = lambda: kv(q, k16, v16, cache_seqlens=sl, max_seqlen_k=cap, causal=True)
    return f8, f16, sum(lens) * Hk * D * 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_fp8_ab.txt"))
    a = ap.parse_args()
    lines = [f"# tools/decode_fp8_ab.py --rounds {a.rounds} --steps {a.steps}: bf16 queries, causal, scale 8, N = 1; median us per call over the "
             f"rounds; MB = valid K+V bytes read; % = share of the copy rate ({COPY_GBS:.0f} GB/s); spread = larger (max - min) of the two calls",
             f"{'shape':34s} {'fp8 us':>8s} {'16b us':>8s} {'16b/fp8':>7s} {'fp8 MB':>8s} {'16b MB':>8s} {'fp8 %':>6s} {'16b %':>6s} {'spread us':>9s}  verdict"]
    ok = True
    torch.manual_seed(0)
    with torch.no_grad():
        for label, B, H, Hk, L, D in SHAPES + [("ragged B8 H32 Hk8 sum 64k D128", 8, 32, 8, RAGGED, 128)]:
            lens = L if isinstance(L, list) else [L] * B
            f8, f16, bytes8 = case(B, H, Hk, lens, D, 1)
            t8s, t16s = ab([f8, f16], a.rounds, a.steps)
            t8, t16 = statistics.median(t8s), statistics.median(t16s)
            spread = max(max(t8s) - min(t8s), max(t16s) - min(t16s))
            good = t8 - t16 <= spread
            ok &= good
            pct = lambda nbytes, t: 100 * nbytes / t / 1e3 / COPY_GBS
            lines.append(f"{label:34s} {t8:8.1f} {t16:8.1f} {t16 / t8:6.2f}x {bytes8 / 1e6:8.1f} {2 * bytes8 / 1e6:8.1f} {pct(bytes8, t8):5.1f}% "
                         f"{pct(2 * bytes8, t16):5.1f}% {spread:9.1f}  {'ok' if good else 'SLOWER'}")
            print(lines[-1], flush=True)
            del f8, f16
            torch.cuda.empty_cache()
    lines.append(f"requirement fp8 not slower than 16-bit by more than the row's spread, every row: {'met' if ok else 'NOT met'}")
    print(lines[-1])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
