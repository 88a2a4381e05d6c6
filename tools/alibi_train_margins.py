#!/usr/bin/env python3
"""Error of `flash_cosine_sim_attention_alibi` next to the error of the route that existed before it --
`flash_cosine_sim_attention(..., attn_bias = band + the materialised ALiBi matrix in the call's dtype)` -- on the same inputs, both
against the float64 oracle on the raw inputs with the exact (float64) bias: the worst figure per dtype and class over the [H]-slopes cases
of tests/alibi_train_cases.EDGE_CASES in the static regime (the attn_bias route has no [B, H] form, and pushes float16 into the per-row-shift
regime by itself); then, for the per-row-shift cases of FORM_CASES, the forward's elementwise excess of both routes on the slices and in the
pass test_gpu_alibi_train.py compares.  Where the new call needs a bar of its own, tests/tolerances_alibi.py takes 1.5 x the attn_bias
route's figure on the slice where the new call is worst.
usage: alibi_train_margins.py   (needs a GPU; prints the table of profiles/alibi_train_tolerance_margins.txt)"""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import flash_cosine_sim_attention_amd as F
import alibi_train_cases as A
import cases as GC
import tolerances as T
from oracle import cosine_sim_oracle as O
from test_window_cpu import band
from test_gpu_kvcache_alibi import alibi_matrix

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    npf = lambda t: t.detach().cpu().double().numpy()
    worst = {}
    for name, dtype, D, B, H, Hk, N, M, left, right, kw, kind in A.EDGE_CASES:
        scale, groups, causal = kw.get("scale", 8.0), kw.get("groups", 1), kw.get("causal", False)
        if kind != "h" or GC.dynamic_shift_regime(dtype, scale, groups, True, False) or (causal and N > M):
            continue
        g = torch.Generator(device="cuda").manual_seed(sum(map(ord, name)))
        rnd = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32).to(DT[dtype])
        q, k, v, do = rnd(B, H, N, D), rnd(B, Hk, M, D), rnd(B, Hk, M, D), rnd(B, H, N, D)
        sl = np.asarray(A.standard_slopes(H), np.float32)
        bias64 = band(N, M, left, right, causal) + alibi_matrix(sl, N, M)
        G = H // Hk
        kr, vr = np.repeat(npf(k[:1]), G, axis=1), np.repeat(npf(v[:1]), G, axis=1)
        okw = dict(scale=scale, groups=groups, causal=causal, l2norm_qk=True, attn_bias=bias64, eps=1e-10)
        ro, _ = O.attention_forward_stats(npf(q[:1]), kr, vr, **okw)
        rdq, rdk, rdv, _ = O.attention_backward(npf(do[:1]), npf(q[:1]), kr, vr, **okw)
        refs = dict(dq=rdq, dk=rdk.reshape(1, Hk, G, M, D).sum(2), dv=rdv.reshape(1, Hk, G, M, D).sum(2))
        bias_t = torch.tensor(bias64, device="cuda").to(DT[dtype])
        for route in ("new", "attn_bias"):
            qq, kk, vv = (t.detach().clone().requires_grad_() for t in (q, k, v))
            if route == "new":
                o = F.flash_cosine_sim_attention_alibi(qq, kk, vv, torch.tensor(sl, device="cuda"), window_size=(left, right), **kw)
            else:
                o = F.flash_cosine_sim_attention(qq, kk, vv, attn_bias=bias_t, **{a: b for a, b in kw.items() if a != "causal"})
            o.backward(do)
            torch.cuda.synchronize()
            rtol = T.FWD_TOL[dtype][1]
            figs = {"fwd-excess": float((np.abs(npf(o[:1]) - ro) - rtol * np.abs(ro)).max(initial=0.0)),
                    "fwd-rel": float(np.linalg.norm(npf(o[:1]) - ro) / np.linalg.norm(ro))}
            for nm, gt in (("dq", qq.grad), ("dk", kk.grad), ("dv", vv.grad)):
                rr = refs[nm]
                figs["grad-" + nm] = float(np.linalg.norm(npf(gt[:1]) - rr) / max(np.linalg.norm(rr), 1e-3 * np.sqrt(rr.size)))
            for cls, x in figs.items():
                key = (dtype, cls, route)
                if x > worst.get(key, (0.0, ""))[0]:
                    worst[key] = (x, name)
    bars = lambda dtype, cls: {"fwd-excess": T.FWD_TOL[dtype][0], "fwd-rel": T.FWD_TOL[dtype][2]}.get(cls, T.GRAD_TOL[dtype])
    print("# tools/alibi_train_margins.py: worst figure per dtype and class, raw inputs against float64 with the exact bias; batch entry 0")
    print(f"{'dtype':<5} {'class':<11} {'new call':>10} {'attn_bias':>10} {'x 1.5':>10} {'bar':>10}  worst case of the new call")
    for dtype in ("bf16", "f16", "f32"):
        for cls in ("fwd-excess", "fwd-rel", "grad-dq", "grad-dk", "grad-dv"):
            n, b = worst.get((dtype, cls, "new"), (float("nan"), "")), worst.get((dtype, cls, "attn_bias"), (float("nan"), ""))
            print(f"{dtype:<5} {cls:<11} {n[0]:>10.3e} {b[0]:>10.3e} {1.5 * b[0]:>10.3e} {bars(dtype, cls):>10.3e}  {n[1]}")


def per_row_section():
    """the per-row-shift regime (logit ranges beyond the static window): forward elementwise excess of both routes on the slices
    test_gpu_alibi_train.py compares, in the pass it compares them in (16-bit: exact math on the 16-bit operands; float32: raw inputs),
    over the per-row cases of alibi_train_cases.FORM_CASES.  The attn_bias route runs one batch entry at a time ([H, N, M] bias with that
    entry's slopes)."""
    import test_gpu_window as TW
    npf = TW._np
    worst, figure = {}, {}
    for name, dtype, D, B, H, Hk, N, M, left, right, kw, kind in A.FORM_CASES:
        scale, groups, causal, l2 = kw.get("scale", 8.0), kw.get("groups", 1), kw.get("causal", False), kw.get("l2norm_qk", True)
        if not GC.dynamic_shift_regime(dtype, scale, groups, l2, False):
            continue
        q, k, v, do = TW.dense_inputs(dtype, B, H, Hk, N, M, D, seed=sum(map(ord, name)), l2norm=l2)
        slopes = torch.tensor(A.standard_slopes(H) if kind == "h" else A.batch_slopes(B, H), dtype=torch.float32, device="cuda")
        with torch.no_grad():
            o_new = F.flash_cosine_sim_attention_alibi(q, k, v, slopes, window_size=(left, right), **kw)
        G = H // Hk
        for b, hk in sorted({(B - 1, Hk - 1), (0, 0)}):
            hs = slice(hk * G, (hk + 1) * G)
            sl = (slopes if slopes.dim() == 1 else slopes[b]).cpu().numpy()
            bias64 = band(N, M, left, right, causal) + alibi_matrix(sl, N, M)
            with torch.no_grad():
                o_old = F.flash_cosine_sim_attention(q[b:b + 1], k[b:b + 1], v[b:b + 1], attn_bias=torch.tensor(bias64, device="cuda").to(DT[dtype]),
                                                     **{x: y for x, y in kw.items() if x != "causal"})
            kr, vr = (np.repeat(npf(t[b:b + 1, hk:hk + 1]), G, axis=1) for t in (k, v))
            ro, _ = O.attention_forward_stats(npf(q[b:b + 1, hs]), kr, vr, operand_dtype=None if dtype == "f32" else dtype, scale=scale, groups=groups,
                                              causal=causal, l2norm_qk=l2, attn_bias=bias64[hs], eps=1e-300)
            rtol = T.FWD_TOL[dtype][1]
            for route, o in (("new", o_new[b:b + 1, hs]), ("attn_bias", o_old[:, hs])):
                x = float((np.abs(npf(o) - ro) - rtol * np.abs(ro)).max(initial=0.0))
                print(f"  {name}[{b},{hk}] {route}: fwd-excess {x:.3e}")
                figure[(f"{name}[{b},{hk}]", route)] = x
                if x > worst.get((dtype, route), (0.0, ""))[0]:
                    worst[(dtype, route)] = (x, f"{name}[{b},{hk}]")
    print("# per-row-shift regime, forward elementwise excess (16-bit: against exact math on the 16-bit operands; float32: raw inputs), worst over")
    print("# the per-row cases of alibi_train_cases.FORM_CASES on the slices the test compares; bar: atol (x 1.6 for float32, test_gpu_window.py)")
    print("# same slice = the attn_bias route on the slice where the NEW call is worst: tests/tolerances_alibi.py takes 1.5 x that figure")
    print(f"{'dtype':<5} {'new call':>10} {'attn_bias':>10} {'same slice':>10} {'x 1.5':>10} {'bar':>10}  worst case: new call | attn_bias route")
    for dtype in ("bf16", "f16", "f32"):
        n, b = worst.get((dtype, "new"), (float("nan"), "")), worst.get((dtype, "attn_bias"), (float("nan"), ""))
        bar = T.FWD_TOL[dtype][0] * (1.6 if dtype == "f32" else 1.0)
        same = figure.get((n[1], "attn_bias"), float("nan"))
        print(f"{dtype:<5} {n[0]:>10.3e} {b[0]:>10.3e} {same:>10.3e} {1.5 * same:>10.3e} {bar:>10.3e}  {n[1]} | {b[1]}")


if __name__ == "__main__":
    main()
    per_row_section()
