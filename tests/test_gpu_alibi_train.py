"""`flash_cosine_sim_attention_alibi` on the GPU: forward o and dq, dk, dv through the public function against the float64 oracle with
attn_bias = band + ALiBi matrix, per (batch, K/V head) slice and per packed sequence, on the table of alibi_train_cases.py (which
test_alibi_forms_cpu.py shows to launch every reachable `*_alibi_kernel` instantiation); the exact identities (zero slopes are the
windowed call bit for bit, a steep causal slope copies v, [H] slopes are their [B, H] expansion); agreement with the cached call that
serves the same model; device slopes and device tables under graph capture.

Tolerances: the bars of tests/tolerances.py with the bias in the reference, used exactly as test_gpu_window.py::compare_slice uses them for
the same kernel forms (raw and operand-faithful passes, the logit-range factor, the two window classes, the emulated-model rule for
gradients of few keys).  tests/tolerances_alibi.py holds the one class that needs a bar of its own -- the forward's elementwise excess in
the per-row-shift regime, bfloat16 and float32 -- and says where it comes from: the attn_bias route on the same inputs, not these kernels.
"""
import numpy as np
import pytest
import torch

import alibi_train_cases as A
import cases as GC
import test_gpu_varlen as TV
import test_gpu_window as TW
import tolerances as T
import tolerances_alibi as TA
from oracle import cosine_sim_oracle as O
from test_gpu_kvcache_alibi import alibi_matrix

pytestmark = pytest.mark.gpu

DT = TW.DT
_np = TW._np


def _F():
    import flash_cosine_sim_attention_amd as F
    return F


def slopes_of(kind, B, H, device="cuda"):
    s = A.standard_slopes(H) if kind == "h" else A.batch_slopes(B, H)
    return torch.tensor(s, dtype=torch.float32, device=device)


def run_alibi(q, k, v, do, slopes, window, kw, **packed):
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    o = _F().flash_cosine_sim_attention_alibi(q, k, v, slopes, window_size=window, **kw, **packed)
    o.backward(do)
    torch.cuda.synchronize()
    return o.detach(), q.grad, k.grad, v.grad


def compare_slice(label, dtype, kw, window, slopes, got, inp, few_keys, seq_factor=1.0):
    """test_gpu_window.py::compare_slice with the ALiBi matrix of the slice's query heads added to the band: one (batch, K/V head) slice
    against the oracle.  got = (o, dq, dk, dv), inp = (q, k, v, do) as float64 arrays, q-side [1, G, N, D], k-side [1, 1, M, D]; slopes:
    the G float32 slopes of the slice's query heads."""
    o, dq, dk, dv = got
    q, k, v, do = inp
    G, N, M = q.shape[1], q.shape[2], k.shape[2]
    scale, groups, l2 = kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True)
    causal = kw.get("causal", False)
    dyn = GC.dynamic_shift_regime(dtype, scale, groups, l2, False)      # the regime of the call WITHOUT slopes: the bias is <= 0
    cond = GC.logit_cond(dtype, scale, groups, l2)
    kr, vr = np.repeat(k, G, axis=1), np.repeat(v, G, axis=1)
    band = TW.band(N, M, *window, causal)
    bias = band + alibi_matrix(slopes, N, M)
    okw = dict(scale=scale, groups=groups, causal=causal, l2norm_qk=l2, attn_bias=bias, eps=1e-300 if dyn else 1e-10)
    atol, rtol, frel = T.FWD_TOL[dtype]
    model_class = few_keys or N <= 2
    _model = []

    def model():
        if not _model:
            em = O.attention_backward_emulated(do, q, kr, vr, dtype, o_saved=o, **{a: b for a, b in okw.items() if a != "eps"})
            _model.append(dict(dq=em[1], dk=em[2].sum(1, keepdims=True), dv=em[3].sum(1, keepdims=True)))
        return _model[0]

    assert all(np.isfinite(x).all() for x in got), label
    fails = []      # every figure is printed and logged before the case is judged

    def judge(cls, measured, bar, what):
        print(f"{label} {what}: {cls} {measured:.3e} (bar {bar:.3e})")
        if not T.check(f"alibi_train/{cls}/{what}", dtype, measured, bar, label):
            fails.append((cls, what, measured, bar))

    passes = (None,) if dtype == "f32" else (dtype,) if dyn else (None, dtype)
    for operand_dtype in passes:
        c = cond if operand_dtype is None else 1.0
        what = "raw" if operand_dtype is None else "operands"
        ro, _ = O.attention_forward_stats(q, kr, vr, operand_dtype=operand_dtype, **okw)
        excess = float((np.abs(o - ro) - rtol * np.abs(ro)).max(initial=0.0))
        fa = atol * c * (max(T.f32_per_row_excess_factor(scale, groups), TW.F32_PER_ROW_EXCESS) if dtype == "f32" and dyn else 1.0)
        if dyn:      # (the one class with a bar of its own: tolerances_alibi.py)
            fa = max(fa, TA.PER_ROW_FWD_EXCESS.get(dtype, 0.0))
        judge("fwd-excess", excess, fa, what)
        fr = TW.BF16_D16_RAW_FWD_REL if (dtype == "bf16" and q.shape[-1] == 16 and operand_dtype is None) else frel
        judge("fwd-rel", TV._rel(o, ro), fr * c * seq_factor, what)
        no_key = (band[0] == 0).sum(axis=1) == 0
        assert (o[:, :, no_key] == 0).all() and (dq[:, :, no_key] == 0).all(), (label, "rows without a visible key must give exact zeros")
        saved = dict(o_saved=o) if operand_dtype is not None else {}
        rdq, rdk, rdv, _ = O.attention_backward(do, q, kr, vr, operand_dtype=operand_dtype, **saved, **okw)
        refs = dict(dq=rdq, dk=rdk.sum(1, keepdims=True), dv=rdv.sum(1, keepdims=True))
        for name, gg in (("dq", dq), ("dk", dk), ("dv", dv)):
            rr = refs[name]
            err = np.linalg.norm(gg - rr)
            floor = (5e-2 if dtype == "f32" else 1e-3) * np.sqrt(rr.size)
            if dtype == "f32" and np.linalg.norm(rr) < floor and err <= 6e-6 * max(1.0, scale / 8.0) * np.sqrt(rr.size):
                continue
            rel = err / max(np.linalg.norm(rr), floor)
            lim = T.GRAD_TOL[dtype] * c * seq_factor
            if model_class or rel > lim:
                lim = max(lim, TW.MODEL_SLACK * np.linalg.norm(model()[name] - rr) / max(np.linalg.norm(rr), floor))
            judge("grad-" + name, rel, lim, what)
    assert not fails, (label, fails)


@pytest.mark.parametrize("name,dtype,D,B,H,Hk,N,M,left,right,kw,kind", A.DENSE_CASES, ids=[c[0] for c in A.DENSE_CASES])
def test_alibi_parity(name, dtype, D, B, H, Hk, N, M, left, right, kw, kind):
    q, k, v, do = TW.dense_inputs(dtype, B, H, Hk, N, M, D, seed=sum(map(ord, name)), l2norm=kw.get("l2norm_qk", True))
    slopes = slopes_of(kind, B, H)
    o, dq, dk, dv = run_alibi(q, k, v, do, slopes, (left, right), kw)
    G = H // Hk
    for b, hk in sorted({(B - 1, Hk - 1), (0, 0)}):
        hs = slice(hk * G, (hk + 1) * G)
        got = tuple(_np(t) for t in (o[b:b + 1, hs], dq[b:b + 1, hs], dk[b:b + 1, hk:hk + 1], dv[b:b + 1, hk:hk + 1]))
        inp = tuple(_np(t) for t in (q[b:b + 1, hs], k[b:b + 1, hk:hk + 1], v[b:b + 1, hk:hk + 1], do[b:b + 1, hs]))
        sl = (slopes if slopes.dim() == 1 else slopes[b])[hs].cpu().numpy()
        compare_slice(f"{name}[{b},{hk}]", dtype, kw, (left, right), sl, got, inp, TW.few_keys((left, right), kw.get("causal", False)))
    for t in (o, dq, dk, dv):
        assert torch.isfinite(t).all()
    if kw.get("causal", False) and N > M:      # rows without a visible key: exact zeros, and no gradient through them
        assert (o[:, :, :N - M] == 0).all() and (dq[:, :, :N - M] == 0).all()


@pytest.mark.parametrize("name,dtype,D,H,Hk,left,right,kw,kind", A.PACKED_CASES, ids=[c[0] for c in A.PACKED_CASES])
def test_alibi_packed_parity(name, dtype, D, H, Hk, left, right, kw, kind):
    lens = list(A.PACKED_LENGTHS)
    q, k, v, do = TV._packed_inputs(dtype, lens, lens, H, Hk, D, seed=sum(map(ord, name)), l2norm=kw.get("l2norm_qk", True))
    slopes = slopes_of(kind, len(lens), H)
    o, dq, dk, dv = run_alibi(q, k, v, do, slopes, (left, right), kw, cu_seqlens_q=TV._cu(lens), cu_seqlens_k=TV._cu(lens))
    cu = np.concatenate([[0], np.cumsum(lens)])
    G = H // Hk
    for t in (o, dq, dk, dv):
        assert torch.isfinite(t).all()
    for s, n in enumerate(lens):
        if n == 0:
            continue
        sq = slice(cu[s], cu[s + 1])
        for hk in range(Hk):
            hs = slice(hk * G, (hk + 1) * G)
            qside = lambda t: _np(t[sq][:, hs]).transpose(1, 0, 2)[None]
            kside = lambda t: _np(t[sq][:, hk:hk + 1]).transpose(1, 0, 2)[None]
            sl = (slopes if slopes.dim() == 1 else slopes[s])[hs].cpu().numpy()
            compare_slice(f"{name}[seq {s},{hk}]", dtype, kw, (left, right), sl, (qside(o), qside(dq), kside(dk), kside(dv)),
                          (qside(q), kside(k), kside(v), qside(do)), TW.few_keys((left, right), True) or n <= 8, seq_factor=4.0 if n < 100 else 1.0)


# ---- exact identities -----------------------------------------------------------------------------------------------------------------------

def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


IDENT = [("bf16", 64, 2, 8, 2, 257, 257, (64, 0), True), ("f16", 128, 2, 8, 8, 100, 300, (129, 64), False), ("f32", 64, 1, 8, 2, 129, 129, (31, 0), True),
         ("f16", 64, 2, 8, 8, 300, 300, (200, -1), False), ("bf16", 128, 8, 30, 30, 300, 300, (64, 0), True)]


@pytest.mark.parametrize("dtype,D,B,H,Hk,N,M,window,causal", IDENT, ids=[f"{c[0]}_d{c[1]}_b{c[2]}h{c[3]}k{c[4]}_n{c[5]}m{c[6]}" for c in IDENT])
def test_zero_slopes_are_the_windowed_call_bit_for_bit(dtype, D, B, H, Hk, N, M, window, causal):
    """fma(-0, |d|, seed) == seed: the same kernels bodies, the same arithmetic"""
    kw = dict(causal=causal, scale=16.0) if (dtype == "f16" and D == 64) else dict(causal=causal)
    q, k, v, do = TW.dense_inputs(dtype, B, H, Hk, N, M, D, seed=5)
    mine = run_alibi(q, k, v, do, torch.zeros(H, device="cuda"), window, kw)
    theirs = TW.run_local(q, k, v, do, window, kw)
    for name, a, b in zip(("o", "dq", "dk", "dv"), mine, theirs):
        assert torch.equal(_bits(a), _bits(b)), name


def test_zero_slopes_are_the_packed_windowed_call_bit_for_bit():
    lens = list(A.PACKED_LENGTHS)
    for dtype, D, H, Hk, window in (("bf16", 64, 8, 2, (64, 0)), ("f16", 128, 8, 8, (31, 0))):
        q, k, v, do = TV._packed_inputs(dtype, lens, lens, H, Hk, D, seed=11)
        cu = TV._cu(lens)
        mine = run_alibi(q, k, v, do, torch.zeros(len(lens), H, device="cuda"), window, dict(causal=True), cu_seqlens_q=cu, cu_seqlens_k=cu)
        qq, kk, vv = (t.detach().clone().requires_grad_() for t in (q, k, v))
        o = _F().flash_cosine_sim_attention_varlen(qq, kk, vv, cu, cu, window_size=window, causal=True)
        o.backward(do)
        for name, a, b in zip(("o", "dq", "dk", "dv"), mine, (o.detach(), qq.grad, kk.grad, vv.grad)):
            assert torch.equal(_bits(a), _bits(b)), (dtype, name)


def test_a_steep_causal_slope_copies_v():
    """slope 50 under causal, N = M, f32: every weight but the row's own key is at most exp(2 scale - 50) of it, far below the forward bar
    (and an exact 0 from a few positions on), so o_i == v_i up to that bar"""
    B, H, N, D = 2, 8, 257, 64
    q, k, v, do = TW.dense_inputs("f32", B, H, H, N, N, D, seed=3)
    o = _F().flash_cosine_sim_attention_alibi(q, k, v, torch.full((H,), 50.0, device="cuda"), causal=True)
    atol, rtol, _ = T.FWD_TOL["f32"]
    excess = float(((o - v).abs() - rtol * v.abs()).max())
    print(f"steep slope: fwd-excess {excess:.3e} (bar {atol:.3e})")
    assert excess <= atol


def test_head_slopes_are_their_batch_expansion_bit_for_bit():
    B, H, Hk, N, M, D = 3, 8, 2, 130, 200, 64
    q, k, v, do = TW.dense_inputs("bf16", B, H, Hk, N, M, D, seed=9)
    s = slopes_of("h", B, H)
    a = run_alibi(q, k, v, do, s, (-1, -1), dict(causal=True))
    b = run_alibi(q, k, v, do, s[None].expand(B, H).contiguous(), (-1, -1), dict(causal=True))
    c = run_alibi(q, k, v, do, s[None].expand(B, H), (-1, -1), dict(causal=True))      # (a stride-0 view)
    for name, x, y, z in zip(("o", "dq", "dk", "dv"), a, b, c):
        assert torch.equal(_bits(x), _bits(y)) and torch.equal(_bits(x), _bits(z)), name


# ---- train / serve ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_training_forward_agrees_with_the_cached_call(dtype):
    """a causal dense call with N = 40 new tokens behind 1020 cached ones, and the cached call that serves the same model on the same data:
    each inside the forward bar against the oracle"""
    B, H, Hk, N, M, D = 2, 8, 2, 40, 1060, 64
    q, k, v, _ = TW.dense_inputs(dtype, B, H, Hk, N, M, D, seed=21)
    slopes = slopes_of("h", B, H)
    F = _F()
    train = F.flash_cosine_sim_attention_alibi(q, k, v, slopes, causal=True)
    qp = q.permute(0, 2, 1, 3).reshape(B * N, H, D).contiguous()
    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda") * N
    serve = F.flash_cosine_sim_attention_alibi_with_kvcache(qp, k.contiguous(), v.contiguous(), cu, max_seqlen_q=N, max_seqlen_k=M, causal=True,
                                                            alibi_slopes=slopes)
    serve = serve.reshape(B, N, H, D).permute(0, 2, 1, 3)
    atol, rtol, frel = T.FWD_TOL[dtype]
    G = H // Hk
    for b, hk in ((0, 0), (B - 1, Hk - 1)):
        hs = slice(hk * G, (hk + 1) * G)
        kr, vr = (np.repeat(_np(t[b:b + 1, hk:hk + 1]), G, axis=1) for t in (k, v))
        bias = TW.band(N, M, -1, -1, True) + alibi_matrix(slopes[hs].cpu().numpy(), N, M)
        ro, _ = O.attention_forward_stats(_np(q[b:b + 1, hs]), kr, vr, scale=8.0, groups=1, causal=True, l2norm_qk=True, attn_bias=bias, eps=1e-10)
        for who, got in (("train", train), ("serve", serve)):
            g = _np(got[b:b + 1, hs])
            excess, rel = float((np.abs(g - ro) - rtol * np.abs(ro)).max()), TV._rel(g, ro)
            print(f"train/serve {dtype} [{b},{hk}] {who}: fwd-excess {excess:.3e} (bar {atol:.3e}) fwd-rel {rel:.3e} (bar {frel:.3e})")
            assert T.check(f"alibi_train/serve/{who}/fwd-excess", dtype, excess, atol) and T.check(f"alibi_train/serve/{who}/fwd-rel", dtype, rel, frel)


# ---- device slopes, device tables, graph capture ----------------------------------------------------------------------------------------------

def test_device_slopes_and_tables_under_graph_capture():
    """nothing of the call reads the slopes or the tables on the host: it captures, and slopes changed in place are picked up on replay"""
    lens = [130, 64, 257]
    H, Hk, D = 8, 2, 64
    q, k, v, _ = TV._packed_inputs("bf16", lens, lens, H, Hk, D, seed=17)
    cu = TV._cu(lens).cuda()
    slopes = slopes_of("bh", len(lens), H)
    F = _F()
    call = lambda: F.flash_cosine_sim_attention_alibi(q, k, v, slopes, causal=True, cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=257, max_seqlen_k=257)
    eager = call().clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        call()      # (warm-up on the side stream, as torch.cuda.graph asks)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(eager))
    slopes.mul_(0.0)
    graph.replay()
    torch.cuda.synchronize()
    plain = F.flash_cosine_sim_attention_alibi(q, k, v, torch.zeros_like(slopes), causal=True, cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=257,
                                               max_seqlen_k=257)
    assert torch.equal(_bits(out), _bits(plain)) and not torch.equal(_bits(out), _bits(eager))
