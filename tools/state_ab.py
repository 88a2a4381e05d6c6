#!/usr/bin/env python3
"""Attention states for training, same-process A/B (device events around the loop).  For each shape it times one forward + backward step of
  (1) the single call, flash_cosine_sim_attention,
  (s) the single call returning the state, flash_cosine_sim_attention_with_lse, with a gradient for the lse,
  (c) the composed route over C = 2, 4, 8 key chunks: one flash_cosine_sim_attention_with_lse per (query chunk, key chunk) and one
      merge_attention_states_with_grad per query chunk -- non-causal: every query sees every key chunk (one query chunk); causal: the
      ring schedule, key chunk j of query chunk i non-causal for j < i, causal for j == i, skipped for j > i,
in rotation, and prints the best step of a few rounds (us).  The composed route is what a context-parallel rank or a blockwise trainer
runs; here every chunk sits on one device, so the figure is its kernel and launch cost, not a speed-up.
usage: state_ab.py [--steps K] [--warmup W] [--rounds R] > profiles/state_ab.txt"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flash_cosine_sim_attention_amd as F  # noqa: E402

SHAPES = [  # B, H, N, D, dtype
    (1, 8, 16384, 128, torch.bfloat16),
    (4, 8, 4096, 64, torch.bfloat16),
]


def measure(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(steps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps * 1e3


def composed(q, k, v, chunks, causal):
    N = q.shape[2]
    c = N // chunks
    if not causal:
        states = [F.flash_cosine_sim_attention_with_lse(q, k[:, :, j * c:(j + 1) * c], v[:, :, j * c:(j + 1) * c]) for j in range(chunks)]
        return F.merge_attention_states_with_grad([s[0] for s in states], [s[1] for s in states])
    outs, lses = [], []
    for i in range(chunks):
        qi = q[:, :, i * c:(i + 1) * c]
        states = [F.flash_cosine_sim_attention_with_lse(qi, k[:, :, j * c:(j + 1) * c], v[:, :, j * c:(j + 1) * c], causal=(j == i))
                  for j in range(i + 1)]
        o, lse = F.merge_attention_states_with_grad([s[0] for s in states], [s[1] for s in states])
        outs.append(o)
        lses.append(lse)
    return torch.cat(outs, dim=2), torch.cat(lses, dim=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}; {args.steps} steps after {args.warmup} warm-up, best of {args.rounds} rounds of the routes in rotation; "
          "us per forward + backward step (device events around the loop); x = step / step of the single call")
    print(f"{'shape':40s} {'route':28s} {'step us':>10s} {'x':>6s}")
    for B, H, N, D, dt in SHAPES:
        for causal in (False, True):
            g = torch.Generator(device="cuda").manual_seed(0)
            q, k, v = (torch.randn(B, H, N, D, device="cuda", dtype=dt, generator=g).requires_grad_() for _ in range(3))
            do = torch.randn(B, H, N, D, device="cuda", dtype=dt, generator=g)
            dlse = torch.randn(B, H, N, device="cuda", generator=g)

            def single():
                q.grad = k.grad = v.grad = None
                F.flash_cosine_sim_attention(q, k, v, causal=causal).backward(do)

            def state():
                q.grad = k.grad = v.grad = None
                o, lse = F.flash_cosine_sim_attention_with_lse(q, k, v, causal=causal)
                torch.autograd.backward([o, lse], [do, dlse])

            def route(chunks):
                def fn():
                    q.grad = k.grad = v.grad = None
                    o, lse = composed(q, k, v, chunks, causal)
                    torch.autograd.backward([o, lse], [do, dlse])
                return fn

            runs = [("(1) single call", single), ("(s) single call with lse", state)] + [(f"(c) {c} key chunks", route(c)) for c in (2, 4, 8)]
            best = {}
            for _ in range(args.rounds):
                for label, fn in runs:
                    t = measure(fn, args.steps, args.warmup)
                    best[label] = min(best.get(label, t), t)
            name = f"B{B} H{H} N{N} D{D} {str(dt)[6:]} causal={int(causal)}"
            for label, _ in runs:
                print(f"{name:40s} {label:28s} {best[label]:10.1f} {best[label] / best['(1) single call']:6.2f}")
            del q, k, v, do, dlse
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
