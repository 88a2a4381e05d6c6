#!/usr/bin/env python3
"""Prompt chunks against a paged MXFP4 cache, three routes on the same logical cache:
  (a) flash_cosine_sim_attention_mxfp4_prefill_with_kvcache -- the multi-wave chunk kernel of csrc/fcsa_prefill_mx.hip;
  (b) flash_cosine_sim_attention_mxfp4_with_kvcache on identical arguments -- the decode kernel at its own split count, the only route
      there was before (a);
  (c) flash_cosine_sim_attention_prefill_with_kvcache on a 16-bit cache holding the dequantised values -- the floor for the math: no
      conversion, four times the bytes.
The protocol is tools/prefill_ab.py's and tools/decode_mxfp4_ab.py's (its timing functions are imported): ONE process, the routes
alternated round by round and warm, pages of 16 through a shuffled block table, causal, every call appends its tokens; per-call time of
`steps` back-to-back calls between HIP events; median, with the min ... max over the rounds as the run-to-run spread.  Every route rotates
over copies of ITS OWN pools, counted from its own bytes per position, so that at least ROTATE_BYTES of cache pass before a buffer comes
round again (at most MAX_COPIES; only the first copy holds the shared logical cache, the others random values of the same kind).
Per row: the three times, (b)/(a) -- above 1 the new call is faster -- with "beyond spreads": whether the gap exceeds the SUM of both
routes' min ... max spreads, (a)/(c), and the largest |o difference| between (a) and (b) on the first copy (0 where (b) runs one split).
No threshold is asserted: the file records what was measured, slower shapes included.
usage: prefill_mxfp4_ab.py [--rounds R] [--steps K] [--out FILE] [--only SUBSTRING]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import flash_cosine_sim_attention_amd as F  # noqa: E402
from prefill_ab import MAX_COPIES, PAGE, ROTATE_BYTES, ROWS as ROWS_16, ab, rotating, visible_pairs  # noqa: E402

ROWS = [r for r in ROWS_16 if r[6]]      # the causal rows of the 16-bit table: the same shapes, row for row


def mx_pool(blocks, Hk, D):
    """(codes, scales) of one pool: random codes, scale bytes 123 ... 129"""
    return (torch.randint(0, 256, (blocks, Hk, PAGE, D // 2), dtype=torch.uint8, device="cuda"),
            torch.randint(123, 130, (blocks, Hk, PAGE, D // 32), dtype=torch.uint8, device="cuda"))


def dense_of(codes, scales, dtype):
    """the pool's values in `dtype`, dequantised 1024 blocks at a time"""
    out = torch.empty(*codes.shape[:3], 2 * codes.shape[3], dtype=dtype, device="cuda")
    for i in range(0, codes.shape[0], 1024):
        out[i:i + 1024] = F.mxfp4_dequantize(codes[i:i + 1024], scales[i:i + 1024], dtype)
    return out


def case(H, Hk, D, counts, cached, dt):
    B, total = len(counts), sum(counts)
    cap = -(-max(c + n for c, n in zip(counts, cached)) // PAGE) * PAGE
    blocks, positions = B * (cap // PAGE), sum(c + n for c, n in zip(counts, cached))
    copies = lambda per_position: min(MAX_COPIES, max(1, -(-int(ROTATE_BYTES) // (positions * Hk * per_position))))
    q = torch.randn(total, H, D, device="cuda", dtype=dt)
    kn, vn = (torch.randn(total, Hk, D, device="cuda", dtype=dt) for _ in range(2))
    cu = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32, device="cuda")
    kw = dict(cache_seqlens=torch.tensor(cached, dtype=torch.int32, device="cuda"), max_seqlen_q=max(counts), max_seqlen_k=cap, causal=True,
              block_table=torch.randperm(blocks, generator=torch.Generator().manual_seed(1)).to(torch.int32).view(B, -1).cuda())
    mx_a, mx_b = ([(mx_pool(blocks, Hk, D), mx_pool(blocks, Hk, D)) for _ in range(copies(2 * (D // 2 + D // 32)))] for _ in range(2))
    for (k, v), (k0, v0) in zip(mx_b[:1], mx_a[:1]):      # the first copy of (b) holds (a)'s cache
        for dst, src in zip(k + v, k0 + v0):
            dst.copy_(src)
    (kc, ks), (vc, vs) = mx_a[0]
    b16 = [(dense_of(kc, ks, dt), dense_of(vc, vs, dt))]
    b16 += [tuple(torch.empty_like(b16[0][0]).normal_() for _ in range(2)) for _ in range(copies(2 * 2 * D) - 1)]
    mx_call = lambda fn, k, v: (lambda: fn(q, k[0], v[0], k[1], v[1], cu_seqlens_q=cu, k_new=kn, v_new=vn, **kw))
    new = [mx_call(F.flash_cosine_sim_attention_mxfp4_prefill_with_kvcache, k, v) for k, v in mx_a]
    old = [mx_call(F.flash_cosine_sim_attention_mxfp4_with_kvcache, k, v) for k, v in mx_b]
    floor = [(lambda k, v: (lambda: F.flash_cosine_sim_attention_prefill_with_kvcache(q, k, v, cu, kn, vn, **kw)))(k, v) for k, v in b16]
    diff = float((new[0]().float() - old[0]().float()).abs().max())
    return rotating(new), rotating(old), rotating(floor), (len(mx_a), len(mx_b), len(b16)), diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefill_mxfp4_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prefill_mxfp4_ab.py measures on the GPU: no GPU visible")
    lines = [f"# tools/prefill_mxfp4_ab.py --rounds {a.rounds} --steps {a.steps}: bf16 (rows named f16: float16), scale 8, causal, paged MXFP4 cache (pages of {PAGE}, "
             "shuffled table), every call appends its tokens; us per call: median (min ... max over the rounds); (a) the chunk kernel, (b) the decode "
             "call on identical arguments, (c) the 16-bit chunk kernel on the dequantised cache; every route rotates over its own pool copies "
             f"(>= {ROTATE_BYTES / 1e6:.0f} MB of cache between two uses of a buffer, at most {MAX_COPIES} copies)",
             f"# device: {torch.cuda.get_device_name(0)}",
             f"{'row':28s} {'copies a/b/c':>12s} {'Mpairs':>8s} {'(a) mxfp4 prefill us':>30s} {'(b) mxfp4 decode us':>32s} {'(c) 16-bit prefill us':>30s} {'(b)/(a)':>8s} "
             f"{'beyond spreads':>14s} {'(a)/(c)':>8s} {'max |diff|':>10s}"]
    print("\n".join(lines), flush=True)
    torch.manual_seed(0)
    fmt = lambda t: f"{t[0]:9.1f} ({t[1]:.1f} ... {t[2]:.1f})"
    with torch.no_grad():
        for name, H, Hk, D, counts, cached, _ in ROWS:
            if a.only not in name:
                continue
            new, old, floor, copies, diff = case(H, Hk, D, counts, cached, torch.float16 if name.startswith("f16") else torch.bfloat16)
            # long rows take fewer steps: a row's timing stays around a second per route and round at most
            pairs = visible_pairs(counts, cached, True)
            t_a, t_b, t_c = ab([new, old, floor], a.rounds, max(3, min(a.steps, int(2e10 / max(pairs * H * D, 1)))))
            spreads = (t_a[2] - t_a[1]) + (t_b[2] - t_b[1])
            verdict = ("faster" if t_b[0] > t_a[0] else "slower") + (", yes" if abs(t_b[0] - t_a[0]) > spreads else ", within")
            lines.append(f"{name:28s} {'/'.join(map(str, copies)):>12s} {pairs / 1e6:8.2f} {fmt(t_a):>30s} {fmt(t_b):>32s} {fmt(t_c):>30s} {t_b[0] / t_a[0]:7.2f}x "
                         f"{verdict:>14s} {t_a[0] / t_c[0]:7.2f}x {diff:10.2e}")
            print(lines[-1], flush=True)
            del new, old, floor
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
