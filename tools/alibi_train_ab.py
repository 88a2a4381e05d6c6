#!/usr/bin/env python3
"""Training with a linear position bias: `flash_cosine_sim_attention_alibi` against what a caller could run before it, interleaved in ONE
process (the protocol of tools/window_ab.py: device events around at least --steps calls and at least 20 ms of work, behind one untimed
call that keeps the queue busy while the host enqueues; round 0 warms every route up).  Routes per row:
  a  the new call (slopes in registers)
  b  flash_cosine_sim_attention(..., attn_bias = the materialised [H, N, M] ALiBi matrix, causal=True), no bias gradient: the best route
     that existed (the causal BIAS forms skip the tiles above the diagonal)
  e  the same with the causal band baked into the bias as -inf and causal=False: every tile visited (what a caller with a window-shaped
     mask in the bias runs); recorded, not part of the condition
  c  the same call without slopes on the same kernel forms (windowed / packed): the cost of the bias itself
  d  the dense causal call without slopes (fwd3 / fwd2 / split forms, which a call with slopes does not take)
Forward and forward + backward; --rounds timings per route, median; the spread of a row is the largest deviation of route a's timings
from their median.  Condition: a faster than b by more than the row's spread on every dense row.  Packed and windowed rows have no b.
usage: alibi_train_ab.py [--rounds R] [--steps S] [--quick]"""
import argparse, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flash_cosine_sim_attention_amd as F

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--quick", action="store_true", help="N = 4096, D = 64 only")
a = ap.parse_args()
_steps = {}


def timed(fn, key):
    """us per call; `key` remembers the step count of a (row, route) so that every round times the same amount of work"""
    steps = _steps.get(key)
    if steps is None:
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); fn(); e1.record()
        torch.cuda.synchronize()
        steps = _steps[key] = max(a.steps, int(20e3 / max(e0.elapsed_time(e1) * 1e3 / 2, 1.0)) + 1)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()                      # untimed: the device is busy while the host enqueues the first timed call
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def spread_of(xs):
    m = statistics.median(xs)
    return max(abs(x - m) for x in xs) / m


def slopes(H):
    return torch.tensor([2.0 ** (-8.0 * (h + 1) / H) for h in range(H)], dtype=torch.float32, device="cuda")


def alibi_bias(H, N, dt, band):
    """[H, N, N] in the call's dtype; band: the keys above the diagonal are -inf (for a call without causal=True)"""
    i = torch.arange(N, device="cuda")[:, None]
    j = torch.arange(N, device="cuda")[None]
    b = -slopes(H)[:, None, None] * (i - j).abs()[None].float()
    if band:
        b = b.masked_fill_((j > i)[None], float("-inf"))
    return b.to(dt).contiguous()


def measure(label, routes, grads):
    """routes: {name: callable returning o}; prints one row, returns {route: (median fwd, median f+b)} and the spreads of route a"""
    def fwd(fn):
        with torch.no_grad():
            fn()

    def fb(fn, do):
        o = fn()
        o.backward(do)
        for t in grads:
            t.grad = None

    do = torch.randn_like(routes["a"]())
    t = {(r, m): [] for r in routes for m in "fb"}
    for rnd in range(a.rounds + 1):
        for r, fn in routes.items():
            f_us, b_us = timed(lambda: fwd(fn), (label, r, "f")), timed(lambda: fb(fn, do), (label, r, "b"))
            if rnd:
                t[(r, "f")].append(f_us); t[(r, "b")].append(b_us)
    med = {k: statistics.median(v) for k, v in t.items()}
    return med, spread_of(t[("a", "f")]), spread_of(t[("a", "b")])


def fmt(med, r, m):
    return f"{med[(r, m)]:>9.1f}" if (r, m) in med else f"{'-':>9}"


def header():
    return (f"{'row':<34} | {'a fwd':>9} {'b fwd':>9} {'e fwd':>9} {'c fwd':>9} {'d fwd':>9} {'b/a':>6} {'e/a':>6} {'a/c':>6} {'a/d':>6} {'spread':>7} | "
            f"{'a f+b':>9} {'b f+b':>9} {'e f+b':>9} {'c f+b':>9} {'d f+b':>9} {'b/a':>6} {'e/a':>6} {'a/c':>6} {'a/d':>6} {'spread':>7}")


def row(label, med, sf, sb):
    ratio = lambda x, y, m: f"{med[(x, m)] / med[(y, m)]:>6.2f}" if (x, m) in med and (y, m) in med else f"{'-':>6}"
    print(f"{label:<34} | {fmt(med, 'a', 'f')} {fmt(med, 'b', 'f')} {fmt(med, 'e', 'f')} {fmt(med, 'c', 'f')} {fmt(med, 'd', 'f')} {ratio('b', 'a', 'f')} "
          f"{ratio('e', 'a', 'f')} {ratio('a', 'c', 'f')} {ratio('a', 'd', 'f')} {sf:>7.1%} | {fmt(med, 'a', 'b')} {fmt(med, 'b', 'b')} {fmt(med, 'e', 'b')} "
          f"{fmt(med, 'c', 'b')} {fmt(med, 'd', 'b')} {ratio('b', 'a', 'b')} {ratio('e', 'a', 'b')} {ratio('a', 'c', 'b')} {ratio('a', 'd', 'b')} {sb:>7.1%}", flush=True)


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    print(f"# tools/alibi_train_ab.py --rounds {a.rounds} --steps {a.steps}: (4, 8, N, D), causal, standard slopes 2^(-8(h+1)/H); median us per call")
    print("# a = flash_cosine_sim_attention_alibi; b = attn_bias route (materialised finite bias, causal=True, no bias gradient); e = attn_bias route")
    print("# with the causal band as -inf in the bias and causal=False; c = the same kernel forms without slopes (a window of N - 2 keys to the left:")
    print("# windowed forms that hide one pair); d = the dense causal call; spread: route a's timings")
    print(header())
    verdict = []
    B, H = 4, 8
    for dt, name in ((torch.bfloat16, "bf16"), (torch.float16, "f16")):
        for D in ((64,) if a.quick else (64, 128)):
            for N in ((4096,) if a.quick else (4096, 8192)):
                q, k, v = (torch.randn(B, H, N, D, device="cuda", dtype=dt, requires_grad=True) for _ in range(3))
                s, bias, band_bias = slopes(H), alibi_bias(H, N, dt, False), alibi_bias(H, N, dt, True)
                routes = dict(a=lambda: F.flash_cosine_sim_attention_alibi(q, k, v, s, causal=True),
                              b=lambda: F.flash_cosine_sim_attention(q, k, v, attn_bias=bias, causal=True),
                              e=lambda: F.flash_cosine_sim_attention(q, k, v, attn_bias=band_bias),
                              c=lambda: F.flash_cosine_sim_attention_local(q, k, v, (N - 2, 0), causal=True),
                              d=lambda: F.flash_cosine_sim_attention(q, k, v, causal=True))
                label = f"{name} D{D} N{N} dense causal"
                med, sf, sb = measure(label, routes, (q, k, v))
                row(label, med, sf, sb)
                verdict.append((label, med[("a", "f")] < med[("b", "f")] * (1 - sf), med[("a", "b")] < med[("b", "b")] * (1 - sb)))
                del bias, band_bias, q, k, v
    bad = [x[0] + (" fwd" if not x[1] else "") + (" fwd+bwd" if not x[2] else "") for x in verdict if not (x[1] and x[2])]
    print(f"condition (a faster than b by more than the row's spread, forward and forward + backward), {len(verdict)} dense rows: "
          f"{'met on all' if not bad else 'NOT met on ' + str(bad)}")
    # one window row and one packed row (no attn_bias route exists for them)
    dt, D, N = torch.bfloat16, 64, 8192
    q, k, v = (torch.randn(B, H, N, D, device="cuda", dtype=dt, requires_grad=True) for _ in range(3))
    s = slopes(H)
    routes = dict(a=lambda: F.flash_cosine_sim_attention_alibi(q, k, v, s, causal=True, window_size=(1024, 0)),
                  c=lambda: F.flash_cosine_sim_attention_local(q, k, v, (1024, 0), causal=True))
    label = f"bf16 D{D} N{N} window (1024, 0)"
    row(label, *measure(label, routes, (q, k, v)))
    del q, k, v
    g = torch.Generator().manual_seed(0)
    lens = [int(x) for x in torch.randint(256, 2048, (32,), generator=g)]
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device="cuda")
    total, mx = sum(lens), max(lens)
    q, k, v = (torch.randn(total, H, D, device="cuda", dtype=dt, requires_grad=True) for _ in range(3))
    routes = dict(a=lambda: F.flash_cosine_sim_attention_alibi(q, k, v, s, causal=True, cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=mx, max_seqlen_k=mx),
                  c=lambda: F.flash_cosine_sim_attention_varlen(q, k, v, cu, cu, max_seqlen_q=mx, max_seqlen_k=mx, causal=True))
    label = f"bf16 D{D} packed 32 docs ({total} rows)"
    row(label, *measure(label, routes, (q, k, v)))


if __name__ == "__main__":
    main()
