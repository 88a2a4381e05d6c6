#!/usr/bin/env python3
"""Decoding against an MXFP4 cache: flash_cosine_sim_attention_mxfp4_with_kvcache against the float8_e4m3fn call and the 16-bit call
(flash_cosine_sim_attention_varlen_with_kvcache) on the SAME logical cache -- the 16-bit pool holds the dequantised MXFP4 values and the fp8
pool their e4m3 codes (scale 1; the scale bytes are drawn from 123 ... 129, so every value is an e4m3 number too).  The protocol and the
shapes are those of tools/decode_alibi_ab.py: ONE process, the calls alternated round by round and warm (bf16, H 32, Hk 8, D 128, paged
caches with pages of 16, causal, every token appends its key and value; per-call time of `--steps` back-to-back calls between HIP events;
median, with the min ... max over the rounds as the run-to-run spread), every route rotating over enough copies of ITS OWN pool -- counted
from its own bytes per position: 512, 256 and 68 -- that at least ROTATE_BYTES of cache pass before a buffer comes round again (only the
first copy of each route holds the shared logical cache; the others hold random values of the same kind).

Per row: the three times, the ratios of medians (above 1: the MXFP4 call is faster), the spread of the 16-bit timings as the yardstick, and
"of copy": the cache bytes the MXFP4 call reads (codes and scale bytes of every cached position, K and V) per second, as a fraction of the
device's copy rate -- bytes read per second by a large device-to-device copy, measured in the same process.
No threshold is asserted: the file records what was measured.
usage: decode_mxfp4_ab.py [--rounds R] [--steps K] [--out FILE]"""
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
SHAPES = [(B, N, L) for L in (4096, 32768) for B in (8, 64) for N in (1, 8)]
ROTATE_BYTES = 600e6


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


def copy_rate():
    """bytes READ per second by a 1 GiB device-to-device copy (it writes as many)"""
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda").zero_()
    dst = torch.empty_like(src)
    us = ab([lambda: dst.copy_(src)], 5, 10)[0][0]
    return src.numel() / (us * 1e-6)


def mx_pool(blocks):
    """(codes, scales) of one pool: random codes, scale bytes 123 ... 129"""
    codes = torch.randint(0, 256, (blocks, HK, PAGE, D // 2), dtype=torch.uint8, device="cuda")
    scales = torch.randint(123, 130, (blocks, HK, PAGE, D // 32), dtype=torch.uint8, device="cuda")
    return codes, scales


def dense_of(codes, scales, dtype):
    """the pool's values in `dtype`, dequantised 1024 blocks at a time"""
    out = torch.empty(*codes.shape[:3], D, dtype=dtype, device="cuda")
    for i in range(0, codes.shape[0], 1024):
        out[i:i + 1024] = F.mxfp4_dequantize(codes[i:i + 1024], scales[i:i + 1024], DT).to(dtype)
    return out


def case(B, N, L):
    pages = L // PAGE
    blocks = B * pages
    mx_bytes = 2 * B * L * HK * (D // 2 + D // 32)
    q = torch.randn(B * N, H, D, device="cuda", dtype=DT)
    kn, vn = (torch.randn(B * N, HK, D, device="cuda", dtype=DT) for _ in range(2))
    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda") * N
    sl = torch.full((B,), L - N, dtype=torch.int32, device="cuda")
    table = torch.randperm(blocks, device="cuda").to(torch.int32).view(B, pages)
    kw = dict(block_table=table, max_seqlen_q=N, max_seqlen_k=L, causal=True)
    copies = lambda nbytes: max(1, -(-int(ROTATE_BYTES) // nbytes))
    mx = [(mx_pool(blocks), mx_pool(blocks)) for _ in range(copies(mx_bytes))]
    (kc, ks), (vc, vs) = mx[0]
    noise = lambda dtype: tuple(torch.empty(blocks, HK, PAGE, D, device="cuda", dtype=DT).normal_().to(dtype) for _ in range(2))
    b16 = [(dense_of(kc, ks, DT), dense_of(vc, vs, DT))] + [noise(DT) for _ in range(copies(mx_bytes * 256 // 68) - 1)]
    fp8 = [tuple(t.to(torch.float8_e4m3fn) for t in b16[0])] + [noise(torch.float8_e4m3fn) for _ in range(copies(mx_bytes * 128 // 68) - 1)]
    r16 = rotating([lambda k=k, v=v: F.flash_cosine_sim_attention_varlen_with_kvcache(q, k, v, cu, kn, vn, sl, **kw) for k, v in b16])
    r8 = rotating([lambda k=k, v=v: F.flash_cosine_sim_attention_varlen_with_kvcache(q, k, v, cu, kn, vn, sl, **kw) for k, v in fp8])
    rmx = rotating([lambda a=a, b=b: F.flash_cosine_sim_attention_mxfp4_with_kvcache(q, a[0], b[0], a[1], b[1], cu_seqlens_q=cu, k_new=kn, v_new=vn,
                                                                                    cache_seqlens=sl, **kw) for a, b in mx])
    return r16, r8, rmx, (len(b16), len(fp8), len(mx)), mx_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_mxfp4_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_mxfp4_ab.py measures on the GPU: no GPU visible")
    torch.manual_seed(0)
    rate = copy_rate()
    lines = [f"# tools/decode_mxfp4_ab.py --rounds {a.rounds} --steps {a.steps}: bf16, H{H} Hk{HK} D{D}, pages of {PAGE}, causal, append; us per call: "
             "median (min ... max over the rounds); the routes rotate over copies of their cache pools "
             f"(>= {ROTATE_BYTES / 1e6:.0f} MB of cache between two uses of a buffer: HBM-resident, not cache-warm)",
             f"# device: {torch.cuda.get_device_name(0)}; copy rate (bytes read per second by a 1 GiB device copy): {rate / 1e9:.0f} GB/s",
             f"{'shape':18s} {'MX MB':>8s} {'copies 16/8/mx':>14s} {'16-bit us':>30s} {'fp8 us':>30s} {'mxfp4 us':>30s} {'16/mx':>8s} {'fp8/mx':>8s} {'16/fp8':>8s} "
             f"{'16-bit spread':>13s} {'mx spread':>9s} {'of copy':>8s}"]
    fmt = lambda t: f"{t[0]:9.1f} ({t[1]:.1f} ... {t[2]:.1f})"
    spread = lambda t: 100 * (t[2] - t[1]) / t[0]
    with torch.no_grad():
        for B, N, L in SHAPES:
            r16, r8, rmx, copies, mx_bytes = case(B, N, L)
            t16, t8, tmx = ab([r16, r8, rmx], a.rounds, a.steps)
            lines.append(f"{f'B{B} N{N} L{L}':18s} {mx_bytes / 1e6:8.1f} {'/'.join(map(str, copies)):>14s} {fmt(t16):>30s} {fmt(t8):>30s} {fmt(tmx):>30s} {t16[0] / tmx[0]:7.3f}x "
                         f"{t8[0] / tmx[0]:7.3f}x {t16[0] / t8[0]:7.3f}x {spread(t16):12.1f}% {spread(tmx):8.1f}% {mx_bytes / (tmx[0] * 1e-6) / rate:8.3f}")
            print(lines[-1], flush=True)
            del r16, r8, rmx
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
