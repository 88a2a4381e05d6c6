#!/usr/bin/env python3
"""The rotary embedding inside the engine step: flash_cosine_sim_attention_rotary_with_kvcache (theta = 10000 tables with one row per cache
position, GPT-NeoX pairs, rotary_dim = D) against the two routes that existed.  The protocol and the shapes are those of
tools/decode_alibi_ab.py: ONE process, the calls alternated round by round and warm (bf16, H 32, Hk 8, D 128, paged caches with pages of
16, causal, every token appends its key and value; per-call time of `--steps` back-to-back calls between HIP events; median, with the
min ... max over the rounds as the run-to-run spread), every route rotating over enough copies of the cache pool that at least
ROTATE_BYTES of keys and values pass before a buffer comes round again.  One more row is a 1024-token prompt chunk.

Per row:
  floor     the step call on q and k_new rotated beforehand, outside the timed region: what the attention itself costs
  composed  what a RoPE user ran before: gather the table rows at cache_seqlens[b] + i, rotate q and k_new with torch in float32, round
            them to the type, step call -- all inside the timed region
  rotary    the new call on the raw q and k_new
"rotary/floor" and "rotary/composed" are ratios of medians; "step spread" is the (max - min) / median of the floor timings, the
yardstick for them.  No threshold is asserted: the file records what was measured.
usage: decode_rotary_ab.py [--rounds R] [--steps K] [--out FILE]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flash_cosine_sim_attention_amd as F  # noqa: E402
from decode_alibi_ab import D, DT, H, HK, PAGE, ROTATE_BYTES, SHAPES, ab, rotating  # noqa: E402

step_call = F.flash_cosine_sim_attention_step_with_kvcache
rotary_call = F.flash_cosine_sim_attention_rotary_with_kvcache


def rotate(x, cos, sin):
    """x [rows, heads, D] by per-row angles cos / sin [rows, D / 2], GPT-NeoX pairs, float32 inside, rounded to x's type"""
    a, b = x.float().chunk(2, dim=-1)
    c, s = cos[:, None], sin[:, None]
    return torch.cat([a * c - b * s, a * s + b * c], dim=-1).to(x.dtype)


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
    ang = torch.arange(L, device="cuda", dtype=torch.float64)[:, None] * 10000.0 ** (-torch.arange(D // 2, device="cuda", dtype=torch.float64) / (D // 2))
    cos, sin = ang.cos().float(), ang.sin().float()
    kw = dict(block_table=table, max_seqlen_q=N, max_seqlen_k=L, causal=True, max_decode_tokens=B * N)
    offsets = torch.arange(N, device="cuda")

    def gathered():      # the rows of a ragged batch: cache_seqlens[b] + i
        pos = (sl.long()[:, None] + offsets[None]).reshape(-1)
        return cos[pos], sin[pos]
    q_rot, k_rot = rotate(q, *gathered()), rotate(kn, *gathered())

    def composed(k, v):
        c, s = gathered()
        return step_call(rotate(q, c, s), k, v, cu, rotate(kn, c, s), vn, sl, **kw)
    floor = rotating([lambda k=k, v=v: step_call(q_rot, k, v, cu, k_rot, vn, sl, **kw) for k, v in pools])
    comp = rotating([lambda k=k, v=v: composed(k, v) for k, v in pools])
    new = rotating([lambda k=k, v=v: rotary_call(q, k, v, cu, kn, vn, sl, rotary_cos=cos, rotary_sin=sin, **kw) for k, v in pools])
    return floor, comp, new, copies, kv_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_rotary_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_rotary_ab.py measures on the GPU: no GPU visible")
    lines = [f"# tools/decode_rotary_ab.py --rounds {a.rounds} --steps {a.steps}: bf16, H{H} Hk{HK} D{D}, rotary_dim {D}, pages of {PAGE}, causal, append; us per "
             f"call: median (min ... max over the rounds); the routes rotate over `copies` cache pools (>= {ROTATE_BYTES / 1e6:.0f} MB of keys and values "
             "between two uses of a buffer: HBM-resident, not cache-warm)",
             f"# device: {torch.cuda.get_device_name(0)}",
             f"{'shape':18s} {'KV MB':>8s} {'copies':>6s} {'floor us':>30s} {'composed us':>30s} {'rotary us':>30s} {'rotary/floor':>12s} "
             f"{'rotary/composed':>15s} {'step spread':>11s}"]
    torch.manual_seed(0)
    fmt = lambda t: f"{t[0]:9.1f} ({t[1]:.1f} ... {t[2]:.1f})"
    with torch.no_grad():
        for B, N, L in SHAPES:
            floor, comp, new, copies, kv_bytes = case(B, N, L)
            t_floor, t_comp, t_new = ab([floor, comp, new], a.rounds, a.steps)
            lines.append(f"{f'B{B} N{N} L{L}':18s} {kv_bytes / 1e6:8.1f} {copies:6d} {fmt(t_floor):>30s} {fmt(t_comp):>30s} {fmt(t_new):>30s} "
                         f"{t_new[0] / t_floor[0]:11.3f}x {t_new[0] / t_comp[0]:14.3f}x {100 * (t_floor[2] - t_floor[1]) / t_floor[0]:10.1f}%")
            print(lines[-1], flush=True)
            del floor, comp, new
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
