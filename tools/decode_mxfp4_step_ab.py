#!/usr/bin/env python3
"""The engine step against an MXFP4 cache: flash_cosine_sim_attention_mxfp4_step_with_kvcache against the route a user had before it --
the packed batch split by hand over flash_cosine_sim_attention_mxfp4_with_kvcache (the decode sequences) and
flash_cosine_sim_attention_mxfp4_prefill_with_kvcache (the chunk sequences), and q / k_new rotated with torch.  The protocol is that of
tools/decode_mxfp4_ab.py and tools/decode_rotary_ab.py: ONE process, the routes alternated round by round and warm (bf16, H 32, Hk 8,
D 128, paged caches with pages of 16, causal, every token appends its key and value; per-call time of `--steps` back-to-back calls between
HIP events; median, with the min ... max over the rounds as the run-to-run spread), the routes rotating over enough copies of the cache pool
that at least ROTATE_BYTES of codes and scale bytes pass before a buffer comes round again: the caches come from HBM.

Rows: pure decodes (64 x 1 token); 63 decodes plus one 512-token chunk; 32 decodes plus one 1024-token chunk; a 1024-token chunk alone --
each on caches of 4k and 32k positions per sequence.  The chunk sits in the MIDDLE of the packed batch, so the hand split needs a gather.
Per row, four routes:
  step       the new call without tables (also the FLOOR of the rotary cost: what the call costs on inputs rotated beforehand)
  split      the hand split: gather the decode rows and the chunk rows of q / k_new / v_new, one decode call and one chunk call (two
             appends), scatter both results -- all inside the timed region; the sub-batches' tables are prepared outside it.  On the two
             rows with ONE kind of sequence there is nothing to split: the route is one direct call of the decode or the chunk function
  step+rope  the new call with tables (theta = 10000, one row per cache position, GPT-NeoX pairs, rotary_dim = D)
  split+rope gather the table rows at cache_seqlens[b] + i, rotate q and k_new with torch in float32, round them to the type, then `split`
"new/old" are ratios of medians (below 1: the new call is faster).  The condition of the feature: on no row is the new call slower than
the old route by more than the two routes' summed spreads (max - min); the verdict column says `ok` or `SLOWER`.  "rope cost" is
step+rope / step.  usage: decode_mxfp4_step_ab.py [--rounds R] [--steps K] [--out FILE]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flash_cosine_sim_attention_amd as F  # noqa: E402
from decode_mxfp4_ab import D, DT, H, HK, PAGE, ROTATE_BYTES, ab, mx_pool, rotating  # noqa: E402

BATCHES = [("64 decodes", 64, None), ("63 dec + 512", 63, 512), ("32 dec + 1024", 32, 1024), ("1024 alone", 0, 1024)]
step_call, dec_call, chunk_call = (F.flash_cosine_sim_attention_mxfp4_step_with_kvcache, F.flash_cosine_sim_attention_mxfp4_with_kvcache,
                                   F.flash_cosine_sim_attention_mxfp4_prefill_with_kvcache)


def rotate(x, cos, sin):
    """x [rows, heads, D] by per-row angles cos / sin [rows, D / 2], GPT-NeoX pairs, float32 inside, rounded to x's type"""
    a, b = x.float().chunk(2, dim=-1)
    c, s = cos[:, None], sin[:, None]
    return torch.cat([a * c - b * s, a * s + b * c], dim=-1).to(x.dtype)


def case(decodes, chunk, L):
    counts = [1] * decodes
    if chunk is not None:
        counts.insert(decodes // 2, chunk)
    B, total, pages = len(counts), sum(counts), L // PAGE
    dev = dict(device="cuda")
    cu_host = [0]
    for n in counts:
        cu_host.append(cu_host[-1] + n)
    cu = torch.tensor(cu_host, dtype=torch.int32, **dev)
    n_b = torch.tensor(counts, dtype=torch.int32, **dev)
    sl = L - n_b
    q = torch.randn(total, H, D, dtype=DT, **dev)
    kn, vn = (torch.randn(total, HK, D, dtype=DT, **dev) for _ in range(2))
    table = torch.randperm(B * pages, **dev).to(torch.int32).view(B, pages)
    mx_bytes = 2 * B * L * HK * (D // 2 + D // 32)
    pools = [(mx_pool(B * pages), mx_pool(B * pages)) for _ in range(max(1, -(-int(ROTATE_BYTES) // mx_bytes)))]
    ang = torch.arange(L, dtype=torch.float64, **dev)[:, None] * 10000.0 ** (-torch.arange(D // 2, dtype=torch.float64, **dev) / (D // 2))
    cos, sin = ang.cos().float(), ang.sin().float()
    kw = dict(block_table=table, max_seqlen_q=max(counts), max_seqlen_k=L, causal=True)
    # the hand split: the sequences of each route, their packed rows, and their own tables (prepared once, outside the timed region)
    seq = torch.arange(B, **dev)
    row_seq = torch.repeat_interleave(seq, n_b.long())
    parts = []
    for name, pick, call in (("dec", n_b == 1, dec_call), ("chunk", n_b > 1, chunk_call)):
        ids = seq[pick]
        if ids.numel() == 0:
            continue
        rows = torch.nonzero(pick[row_seq]).flatten()
        sub_n = n_b[ids]
        sub_cu = torch.cat([torch.zeros(1, dtype=torch.int32, **dev), sub_n.cumsum(0).to(torch.int32)])
        parts.append((call, rows, sub_cu, sl[ids].contiguous(), table[ids].contiguous(), int(sub_n.max())))
    pos = torch.cat([sl[b].long() + torch.arange(n, **dev) for b, n in enumerate(counts)])      # cache_seqlens[b] + i of every packed row

    def split(a, b, qq, kk):
        if len(parts) == 1:      # one kind of sequence: nothing to split -- the one function, called directly on the whole batch
            return parts[0][0](qq, a[0], b[0], a[1], b[1], cu_seqlens_q=cu, k_new=kk, v_new=vn, cache_seqlens=sl, **kw)
        out = torch.empty_like(q)
        for call, rows, sub_cu, sub_sl, sub_table, max_q in parts:
            out[rows] = call(qq[rows], a[0], b[0], a[1], b[1], cu_seqlens_q=sub_cu, k_new=kk[rows], v_new=vn[rows], cache_seqlens=sub_sl,
                             block_table=sub_table, max_seqlen_q=max_q, max_seqlen_k=L, causal=True)
        return out

    def split_rope(a, b):
        c, s = cos[pos], sin[pos]
        return split(a, b, rotate(q, c, s), rotate(kn, c, s))
    # max_decode_tokens: the decode-routed rows, which an engine knows from its scheduler (the tables here are device tensors, so the call
    # cannot count them); without it the split count is sized as if every packed row decoded -- see the note at the end of the profile
    new = lambda a, b, **rope: step_call(q, a[0], b[0], a[1], b[1], cu_seqlens_q=cu, k_new=kn, v_new=vn, cache_seqlens=sl, max_decode_tokens=decodes,
                                         **kw, **rope)
    routes = [rotating([lambda a=a, b=b: new(a, b) for a, b in pools]), rotating([lambda a=a, b=b: split(a, b, q, kn) for a, b in pools]),
              rotating([lambda a=a, b=b: new(a, b, rotary_cos=cos, rotary_sin=sin) for a, b in pools]),
              rotating([lambda a=a, b=b: split_rope(a, b) for a, b in pools])]
    return routes, len(pools), mx_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_mxfp4_step_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_mxfp4_step_ab.py measures on the GPU: no GPU visible")
    torch.manual_seed(0)
    lines = [f"# tools/decode_mxfp4_step_ab.py --rounds {a.rounds} --steps {a.steps}: bf16, H{H} Hk{HK} D{D}, pages of {PAGE}, causal, append, chunk_rows default; "
             f"us per call: median (min ... max over the rounds); the routes rotate over copies of the cache pool (>= {ROTATE_BYTES / 1e6:.0f} MB "
             "between two uses of a buffer: HBM-resident, not cache-warm)",
             f"# device: {torch.cuda.get_device_name(0)}",
             f"{'batch':14s} {'cache':>6s} {'copies':>6s} {'step us':>28s} {'split us':>28s} {'new/old':>8s} {'verdict':>7s} {'step+rope us':>28s} {'split+rope us':>28s} "
             f"{'new/old':>8s} {'verdict':>7s} {'rope cost':>9s}"]
    fmt = lambda t: f"{t[0]:9.1f} ({t[1]:.1f} ... {t[2]:.1f})"
    verdict = lambda new, old: "ok" if new[0] - old[0] <= (new[2] - new[1]) + (old[2] - old[1]) else "SLOWER"
    slower = 0
    with torch.no_grad():
        for L in (4096, 32768):
            for name, decodes, chunk in BATCHES:
                routes, copies, _ = case(decodes, chunk, L)
                ts, to, trs, tro = ab(routes, a.rounds, a.steps)
                slower += (verdict(ts, to) != "ok") + (verdict(trs, tro) != "ok")
                lines.append(f"{name:14s} {L:6d} {copies:6d} {fmt(ts):>28s} {fmt(to):>28s} {ts[0] / to[0]:7.3f}x {verdict(ts, to):>7s} {fmt(trs):>28s} {fmt(tro):>28s} "
                             f"{trs[0] / tro[0]:7.3f}x {verdict(trs, tro):>7s} {trs[0] / ts[0]:8.3f}x")
                print(lines[-1], flush=True)
                del routes
                torch.cuda.empty_cache()
    lines.append(f"# rows on which the new call is slower than the old route by more than the two summed spreads: {slower} of 16")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
