#!/usr/bin/env python3
"""Packed variable-length sequences against the dense op: fwd+bwd step times in ONE process, the calls alternated round by round
(bf16, H = 8, D = 64, scale 8; median and min over the rounds of the per-step time of `--steps` back-to-back steps, HIP events).

  1. S equal-length sequences: flash_cosine_sim_attention_varlen against the dense [S, H, L, D] call -- (4, 4096) causal, (8, 2048)
     non-causal.  Target: within 3 % of dense.
  2. a ragged mix, 32 documents of lengths uniform in [256, 4096] (seeded): varlen against the padded dense call (causal: right padding;
     non-causal: a key mask).  Target (causal): at most 0.5x the padded step.
  3. the worst case for the grid sized by max_seqlen: one 16384-token document and 1024 documents of 16 tokens.  Reported, not gated:
     next to it the dense calls of the two shapes on their own ([1, H, 16384] + [1024, H, 16]), what a compact (sequence, tile) work list
     could approach.
usage: varlen_ab.py [--rounds R] [--steps K] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flash_cosine_sim_attention_amd as F  # noqa: E402

H, D, DT = 8, 64, torch.bfloat16


def cu_of(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device="cuda")


def varlen_step(lens, causal):
    T = int(sum(lens))
    q, k, v = (torch.randn(T, H, D, device="cuda", dtype=DT, requires_grad=True) for _ in range(3))
    do = torch.randn(T, H, D, device="cuda", dtype=DT)
    cu, mx = cu_of(lens), int(max(lens))

    def step():
        o = F.flash_cosine_sim_attention_varlen(q, k, v, cu, cu, max_seqlen_q=mx, max_seqlen_k=mx, causal=causal)
        torch.autograd.grad(o, (q, k, v), do)
    return step


def dense_step(B, L, causal, mask=None):
    q, k, v = (torch.randn(B, H, L, D, device="cuda", dtype=DT, requires_grad=True) for _ in range(3))
    do = torch.randn(B, H, L, D, device="cuda", dtype=DT)

    def step():
        o = F.flash_cosine_sim_attention(q, k, v, mask=mask, causal=causal)
        torch.autograd.grad(o, (q, k, v), do)
    return step


def padded_mask(lens, L):
    return torch.arange(L, device="cuda")[None, :] < torch.tensor(lens, device="cuda")[:, None]


def time_alternated(variants, rounds, steps):
    """{name: [per-step ms of each round]}, the variants run one after the other inside every round"""
    res = {n: [] for n in variants}
    for f in variants.values():          # warm-up: allocator, kernel first launches
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for n, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                f()
            e1.record()
            e1.synchronize()
            res[n].append(e0.elapsed_time(e1) / steps)
    return res


def fmt(res):
    return "  ".join(f"{n} {statistics.median(v):8.3f} ({min(v):8.3f}) ms" for n, v in res.items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    torch.manual_seed(0)
    lines = [f"varlen_ab: bf16, H = {H}, D = {D}, fwd+bwd per step; median (min) over {a.rounds} alternated rounds of {a.steps} steps",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def report(title, res, ratio_of, target=None):
        med = {n: statistics.median(v) for n, v in res.items()}
        r = med[ratio_of[0]] / med[ratio_of[1]]
        verdict = "" if target is None else ("  target " + target[0] + (": met" if target[1](r) else ": NOT met"))
        lines.extend([title, "  " + fmt(res), f"  {ratio_of[0]} / {ratio_of[1]} = {r:.3f}{verdict}", ""])
        print("\n".join(lines[-4:]), flush=True)

    # 1. equal lengths
    for S, L, causal in ((4, 4096, True), (8, 2048, False)):
        res = time_alternated({"dense": dense_step(S, L, causal), "varlen": varlen_step([L] * S, causal)}, a.rounds, a.steps)
        report(f"1. equal lengths S = {S}, L = {L}, {'causal' if causal else 'non-causal'}", res, ("varlen", "dense"),
               ("<= 1.03", lambda r: r <= 1.03))
    # 2. ragged mix against padding
    lens = np.random.default_rng(0).integers(256, 4097, size=32).tolist()
    L = max(lens)
    work_c = sum(-(-n // 128) * (-(-n // 128) + 1) // 2 for n in lens) / (32 * (-(-L // 128)) * (-(-L // 128) + 1) // 2)
    lines.append(f"2. ragged mix: 32 documents, lengths uniform in [256, 4096] (seed 0): {sum(lens)} tokens, longest {L}; "
                 f"causal 128-tile pairs of the packed batch = {work_c:.2f} of the padded batch's")
    res = time_alternated({"padded": dense_step(32, L, True), "varlen": varlen_step(lens, True)}, a.rounds, a.steps)
    report("   causal, right padding", res, ("varlen", "padded"), ("<= 0.50", lambda r: r <= 0.5))
    res = time_alternated({"padded": dense_step(32, L, False, padded_mask(lens, L)), "varlen": varlen_step(lens, False)}, a.rounds, a.steps)
    report("   non-causal, key mask", res, ("varlen", "padded"))
    # 3. one long document and many short ones: most workgroups of the max-sized grid exit at once
    lens = [16384] + [16] * 1024
    for causal in (True, False):
        big, small = dense_step(1, 16384, causal), dense_step(1024, 16, causal)
        res = time_alternated({"varlen": varlen_step(lens, causal), "dense_1x16384+1024x16": lambda: (big(), small())}, a.rounds, a.steps)
        report(f"3. one 16384-token document + 1024 of 16 tokens, {'causal' if causal else 'non-causal'} (reported, not gated)", res,
               ("varlen", "dense_1x16384+1024x16"))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
