#!/usr/bin/env python3
"""The engine step against a paged key/value cache: flash_cosine_sim_attention_step_with_kvcache (every sequence on the kernel built for its
row count) against the two single-kernel calls on the same batch -- flash_cosine_sim_attention_varlen_with_kvcache (the ragged decode
kernel at its own split count) and, wherever it accepts the arguments, flash_cosine_sim_attention_prefill_with_kvcache.
tools/prefill_ab.py's protocol: ONE process, the routes alternated round by round and warm; bf16, scale 8, causal, pages of 16 through a
shuffled block table, every call appends its tokens; per-call time of `--steps` back-to-back calls between HIP events; the median, with the
min ... max over the rounds as the run-to-run spread.  Every route rotates over copies of its caches -- at least ROTATE_BYTES of keys and
values before a buffer comes round again (more than the 256 MB last-level cache), at most MAX_COPIES of them -- so the figures are those of
caches coming from HBM.
Routes of a row: "step" = device tables with max_decode_tokens set to the decode rows (what an engine knows without reading a table);
"step host" = host cu_seqlens_q (the bound is exact and a launch without work is skipped); "ragged"; "prefill".  "x best other" = the faster
of ragged / prefill over the step route: above 1 the step call is faster; "beyond spread": whether that gap exceeds the larger of the two
routes' min ... max spreads.  The mixed rows sweep chunk_rows (host tables) to place the default; rows with chunks and no window time the
always-windowed chunk form (a window of 2^27 keys to the left hides nothing and takes that form) against the plain one, every sequence on
the chunk kernel.  Before timing, the step call is compared with the ragged call on the same inputs (max |diff|).
No threshold is asserted: the file records what was measured, slower shapes included.
usage: step_ab.py [--rounds R] [--steps K] [--out FILE] [--only SUBSTRING]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flash_cosine_sim_attention_amd as F  # noqa: E402
from flash_cosine_sim_attention_amd import _lib  # noqa: E402

DT = torch.bfloat16
PAGE = 16
ROTATE_BYTES = 600e6
MAX_COPIES = 12
SWEEP = (128, 256, 512, 1024, 2048)
HIDES_NOTHING = (1 << 27, -1)

# name, H, Hk, D, query counts, cached positions, fp8, window, mixed (sweeps chunk_rows)
ROWS = [
    ("63 x N1 + N512 on 4k", 32, 8, 128, [1] * 63 + [512], [4096] * 64, False, None, True),
    ("32 x N1 + N1024 on 8k", 32, 8, 128, [1] * 32 + [1024], [8192] * 33, False, None, True),
    ("63 x N1 + N256 on 4k", 32, 8, 128, [1] * 63 + [256], [4096] * 64, False, None, True),
    ("60 x N1 + 4 x N8 on 8k", 32, 8, 128, [1] * 60 + [8] * 4, [8192] * 64, False, None, True),
    ("64 x N1 on 8k", 32, 8, 128, [1] * 64, [8192] * 64, False, None, False),
    ("8 x N512 on 4k", 32, 8, 128, [512] * 8, [4096] * 8, False, None, False),
    ("N64 on 32k", 32, 8, 128, [64], [32768], False, None, False),
    ("fp8 N1024 on 8k", 32, 8, 128, [1024], [8192], True, None, False),
    ("N1024 on 32k left 4096", 32, 8, 128, [1024], [32768], False, (4096, -1), False),
    ("D64 H8/Hk8 63 x N1 + N512 on 4k", 8, 8, 64, [1] * 63 + [512], [4096] * 64, False, None, True),
]


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


def case(H, Hk, D, counts, cached, fp8, window, mixed):
    """{route name: callable} of a row, and the step call's max |diff| against the ragged call"""
    B, total, G = len(counts), sum(counts), H // Hk
    cap = -(-max(c + n for c, n in zip(counts, cached)) // PAGE) * PAGE
    mb = cap // PAGE
    kv_bytes = sum(c + n for c, n in zip(counts, cached)) * Hk * D * 2 * (1 if fp8 else 2)
    copies = min(MAX_COPIES, max(1, -(-int(ROTATE_BYTES) // kv_bytes)))
    q = torch.randn(total, H, D, device="cuda", dtype=DT)
    kn, vn = (torch.randn(total, Hk, D, device="cuda", dtype=DT) for _ in range(2))
    cu_host = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32)
    cu = cu_host.cuda()
    sl = torch.tensor(cached, dtype=torch.int32, device="cuda")
    table = torch.randperm(B * mb, generator=torch.Generator().manual_seed(1)).to(torch.int32).view(B, mb).cuda()
    kw = dict(cache_seqlens=sl, block_table=table, max_seqlen_q=max(counts), max_seqlen_k=cap, causal=True)
    if fp8:
        kw.update(k_scale=torch.full((B, Hk), 0.02, device="cuda"), v_scale=torch.full((B, Hk), 0.02, device="cuda"))
    win = dict(window_size=window) if window else {}

    def pools():
        if fp8:
            return tuple((torch.randn(B * mb, Hk, PAGE, D, device="cuda") * 40).to(torch.float8_e4m3fn) for _ in range(2))
        return tuple(torch.randn(B * mb, Hk, PAGE, D, device="cuda", dtype=DT) for _ in range(2))

    first = pools()
    sets = [first] + [tuple(t.clone() for t in first) for _ in range(copies - 1)]      # same values, other memory

    def route(fn, table_cu, **more):
        return rotating([(lambda k, v: (lambda: fn(q, k, v, table_cu, kn, vn, **kw, **more)))(k, v) for k, v in sets])

    step, ragged, prefill = (F.flash_cosine_sim_attention_step_with_kvcache, F.flash_cosine_sim_attention_varlen_with_kvcache,
                             F.flash_cosine_sim_attention_prefill_with_kvcache)
    decode_rows = sum(n for n in counts if G * n < _lib.STEP_CHUNK_ROWS)
    routes = {"step": route(step, cu, max_decode_tokens=decode_rows, **win), "step host": route(step, cu_host, **win), "ragged": route(ragged, cu, **win)}
    if not fp8 and not window:
        routes["prefill"] = route(prefill, cu)
    if mixed:
        for t in SWEEP:
            routes[f"chunk_rows {t}"] = route(step, cu_host, chunk_rows=t)
    if not window and not fp8 and max(counts) * G >= 128:
        routes["all chunks, plain form"] = route(step, cu_host, chunk_rows=0)
        routes["all chunks, windowed form"] = route(step, cu_host, chunk_rows=0, window_size=HIDES_NOTHING)
    diff = float((routes["step"]().float() - routes["ragged"]().float()).abs().max())
    return routes, copies, diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("step_ab.py measures on the GPU: no GPU visible")
    lines = [f"# tools/step_ab.py --rounds {a.rounds} --steps {a.steps}: bf16, scale 8, causal, paged cache (pages of {PAGE}, shuffled table), every call appends "
             "its tokens; us per call: median (min ... max over the rounds); every route rotates over `copies` sets of caches "
             f"(>= {ROTATE_BYTES / 1e6:.0f} MB of keys and values between two uses of a buffer, at most {MAX_COPIES} sets)",
             f"# device: {torch.cuda.get_device_name(0)}; default chunk_rows: {_lib.STEP_CHUNK_ROWS}"]
    print("\n".join(lines), flush=True)
    torch.manual_seed(0)
    fmt = lambda t: f"{t[0]:9.1f} ({t[1]:.1f} ... {t[2]:.1f})"
    with torch.no_grad():
        for name, H, Hk, D, counts, cached, fp8, window, mixed in ROWS:
            if a.only not in name:
                continue
            routes, copies, diff = case(H, Hk, D, counts, cached, fp8, window, mixed)
            res = dict(zip(routes, ab(list(routes.values()), a.rounds, a.steps)))
            others = {k: res[k] for k in ("ragged", "prefill") if k in res}
            best = min(others, key=lambda k: others[k][0])
            t_s, t_b = res["step"], others[best]
            spread = max(t_s[2] - t_s[1], t_b[2] - t_b[1])
            verdict = ("faster" if t_b[0] > t_s[0] else "slower") + (", beyond spread" if abs(t_b[0] - t_s[0]) > spread else ", within spread")
            lines.append(f"{name}   (copies {copies}, max |step - ragged| {diff:.2e})")
            for k, t in res.items():
                lines.append(f"    {k:28s} {fmt(t):>34s} us   step / this = {t_s[0] / t[0]:5.2f}")
            lines.append(f"    x best other ({best}): {t_b[0] / t_s[0]:.2f}x  {verdict}")
            if "all chunks, windowed form" in res:
                p, w = res["all chunks, plain form"], res["all chunks, windowed form"]
                sp = max(p[2] - p[1], w[2] - w[1])
                lines.append(f"    windowed form / plain form: {w[0] / p[0]:.3f}  ({'within' if abs(w[0] - p[0]) <= sp else 'beyond'} the spread of {sp:.1f} us)")
            print("\n".join(lines[-(len(res) + 3):]), flush=True)
            del routes
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
