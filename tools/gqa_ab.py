#!/usr/bin/env python3
"""Grouped-query attention, same-process A/B (library HIP events, fcsa_profile_*).  For each shape (B, H, Hk, N, D, dtype, causal) it times
one forward + backward step of
  (a) the GQA call, automatic dK/dV form (fcsa_debug_kv_group_form 1),
  (b) the GQA call pinned to the slab route (form 0: per-query-head f32 dK / dV slabs + finalize),
  (s) the GQA call pinned to the group sweep (form 2; where it is compiled: 16-bit D = 64 / 128),
  (c) the same problem with K/V repeat_interleave'd to H heads, called with Hk == H, plus the group sum of its dk / dv (what a caller
      without GQA support pays: the repeat, the H-head backward, the sum),
and prints per-kernel times (us per step) and the step time of the best of a few rounds.  usage: gqa_ab.py [--steps K] [--warmup W] [--rounds R]"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flash_cosine_sim_attention_amd as F  # noqa: E402
from flash_cosine_sim_attention_amd import _lib  # noqa: E402

SHAPES = [  # B, H, Hk, N, D, dtype, causal
    (4, 32, 8, 4096, 64, torch.bfloat16, True),
    (4, 32, 8, 4096, 64, torch.bfloat16, False),
    (2, 32, 4, 4096, 128, torch.bfloat16, True),
    (1, 16, 2, 8192, 64, torch.bfloat16, True),
    (4, 8, 2, 4096, 64, torch.float16, False),
]


def measure(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    t0 = time.perf_counter()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(steps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    st = {s["name"]: s["total_ms"] / steps * 1e3 for s in _lib.profile_collect()}
    _lib.profile_enable(False)
    return ev0.elapsed_time(ev1) / steps * 1e3, wall / steps * 1e6, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}; {args.steps} steps after {args.warmup} warm-up, best of {args.rounds} rounds of the forms in rotation; us per step (device events around the "
          f"loop) and per-kernel us per step (library events; 'finalize' = slab reduction)")
    kernels = ("l2norm", "fwd", "bwd_dq", "bwd_dkv", "finalize")
    print(f"{'shape':44s} {'form':10s} {'step':>9s} " + " ".join(f"{k:>9s}" for k in kernels) + f" {'other':>9s}")
    for B, H, Hk, N, D, dt, causal in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        q = torch.randn(B, H, N, D, device="cuda", dtype=dt, generator=g).requires_grad_()
        k = torch.randn(B, Hk, N, D, device="cuda", dtype=dt, generator=g).requires_grad_()
        v = torch.randn(B, Hk, N, D, device="cuda", dtype=dt, generator=g).requires_grad_()
        do = torch.randn(B, H, N, D, device="cuda", dtype=dt, generator=g)
        G = H // Hk

        def gqa():
            q.grad = k.grad = v.grad = None
            F.flash_cosine_sim_attention(q, k, v, causal=causal).backward(do)

        def expanded():
            q.grad = k.grad = v.grad = None
            ke = k.detach().repeat_interleave(G, 1).requires_grad_()
            ve = v.detach().repeat_interleave(G, 1).requires_grad_()
            F.flash_cosine_sim_attention(q, ke, ve, causal=causal).backward(do)
            ke.grad.view(B, Hk, G, N, D).sum(2)
            ve.grad.view(B, Hk, G, N, D).sum(2)

        name = f"B{B} H{H} Hk{Hk} N{N} D{D} {str(dt)[6:]} causal={int(causal)}"
        runs = [("(a) auto", 1, gqa), ("(b) slabs", 0, gqa)]
        if dt in (torch.float16, torch.bfloat16) and D in (64, 128):
            runs.append(("(s) sweep", 2, gqa))
        runs.append(("(c) expand", 1, expanded))
        best = {}
        for _ in range(args.rounds):      # the forms in rotation, best step of the rounds: the first run of a shape also pays the clock ramp
            for label, form, fn in runs:
                prev = _lib.kv_group_form(form)
                try:
                    res = measure(fn, args.steps, args.warmup)
                finally:
                    _lib.kv_group_form(prev)
                if label not in best or res[0] < best[label][0]:
                    best[label] = res
        for label, _, _ in runs:
            step, _, st = best[label]
            other = step - sum(st.get(kk, 0.0) for kk in kernels)
            print(f"{name:44s} {label:10s} {step:9.1f} " + " ".join(f"{st.get(kk, 0.0):9.1f}" for kk in kernels) + f" {other:9.1f}")
        del q, k, v, do
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
