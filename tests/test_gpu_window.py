"""Sliding-window attention on the GPU (flash_cosine_sim_attention_local, window_size of the packed and decode functions).

The yardstick is the float64 oracle, unchanged: a window is an additive bias of 0 inside the band and -inf outside it, which
attention_forward_stats / attention_backward / attention_backward_emulated take as they are.  Bars: tests/tolerances.py as they stand
(FWD_TOL, GRAD_TOL), the two comparisons of the 16-bit types (exact math on the raw inputs with the bars scaled by cases.logit_cond; exact
math on the 16-bit operands with the fixed bars and the stored output), and the model rule of test_gpu_fuzz.py for ill-conditioned
problems -- a window of a few keys under many rows is that class: a gradient may sit at max(stated bar, 2 x the error of the
working-precision model of the same problem).  The case table is tests/window_cases.py; test_window_forms_cpu.py checks that it launches
every reachable windowed instantiation.  Chip-filling cases run the oracle on two (batch, K/V head) slices.
Identities are bit for bit: (-1, -1) is the un-windowed call, (-1, 0) the causal one, a window that hides nothing the un-windowed one."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases as GC
import test_gpu_kvcache as TK
import test_gpu_varlen as TV
import tolerances as T
import varlen_form_cases as VF
import window_cases as W
from oracle import cosine_sim_oracle as O

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
MODEL_SLACK = 2.0      # test_gpu_fuzz.py kModelSlack
# Two classes of the new cases need a bar of their own (profiles/window_tolerance_margins.txt: <= 1.5 x the worst value measured over
# this file's cases, derived as the bars of tests/tolerances.py were); every other comparison uses those bars as they stand.
#   bf16, D = 16, forward rel-L2 against exact math on the RAW inputs: the un-windowed suite already sits at 4.09e-3 of its 4.5e-3 there
#     (D = 16: few, large components of q^, k^, so their 16-bit rounding moves the logits most); the windowed cases measure up to 5.13e-3,
#     on a case whose rows see up to 1060 keys as well as on one whose rows see at most 127 -- so the class is the head dim, not the
#     window's width, and the bar goes with every bf16 D = 16 raw comparison of this file.  The operand-faithful comparison of the same
#     cases keeps the stated bar.
#   float32 in the per-row-shift regime, elementwise forward excess: tolerances.f32_per_row_excess_factor gives 1.25e-5 at scale x groups
#     = 80 from the packed cases (worst 1.13e-5 there); the windowed cases measure up to 1.44e-5.
BF16_D16_RAW_FWD_REL = 7.5e-3
F32_PER_ROW_EXCESS = 1.6


def _np(t):
    return t.detach().cpu().double().numpy()


def _F():
    import flash_cosine_sim_attention_amd as F
    return F


def band(N, M, left, right, causal):
    """the window as an additive bias [1, N, M]: 0 inside the band, -inf outside"""
    i = np.arange(N)[:, None] + (M - N)
    j = np.arange(M)[None]
    ok = np.ones((N, M), bool)
    if left >= 0:
        ok &= j >= i - left
    r = 0 if causal else right
    if r >= 0:
        ok &= j <= i + r
    return np.where(ok, 0.0, -np.inf)[None]


def dense_inputs(dtype, B, H, Hk, N, M, D, seed, l2norm=True):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32)
    q, k, v, do = rnd(B, H, N, D), rnd(B, Hk, M, D), rnd(B, Hk, M, D), rnd(B, H, N, D)
    if not l2norm:
        q, k = torch.nn.functional.normalize(q, dim=-1), torch.nn.functional.normalize(k, dim=-1)
    return tuple(t.to(DT[dtype]) for t in (q, k, v, do))


def run_local(q, k, v, do, window, kw):
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    o = _F().flash_cosine_sim_attention_local(q, k, v, window, **kw)
    o.backward(do)
    torch.cuda.synchronize()
    return o.detach(), q.grad, k.grad, v.grad


def compare_slice(label, dtype, kw, window, got, inp, few_keys, seq_factor=1.0):
    """one (batch, K/V head) slice against the oracle.  got = (o, dq, dk, dv) and inp = (q, k, v, do) as float64 arrays with q-side
    shapes [1, G, N, D] and k-side [1, 1, M, D] (the group's query heads against their one K/V head)."""
    o, dq, dk, dv = got
    q, k, v, do = inp
    G, N, M = q.shape[1], q.shape[2], k.shape[2]
    scale, groups, l2 = kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True)
    causal = kw.get("causal", False)
    dyn = GC.dynamic_shift_regime(dtype, scale, groups, l2, False)
    cond = GC.logit_cond(dtype, scale, groups, l2)
    kr, vr = np.repeat(k, G, axis=1), np.repeat(v, G, axis=1)
    okw = dict(scale=scale, groups=groups, causal=causal, l2norm_qk=l2, attn_bias=np.repeat(band(N, M, *window, causal), G, axis=0),
               eps=1e-300 if dyn else 1e-10)
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
        if not T.check(f"window/{cls}/{what}", dtype, measured, bar, label):
            fails.append((cls, what, measured, bar))

    # 16-bit types in the per-row-shift regime: exact math on the 16-bit operands only, as test_gpu_varlen.py compares the same kernel
    # forms there (the rounding of c1 * q^ alone moves a logit of range +-80 by more than the raw-input bars allow)
    passes = (None,) if dtype == "f32" else (dtype,) if dyn else (None, dtype)
    for operand_dtype in passes:
        c = cond if operand_dtype is None else 1.0
        what = "raw" if operand_dtype is None else "operands"
        ro, _ = O.attention_forward_stats(q, kr, vr, operand_dtype=operand_dtype, **okw)
        excess = float((np.abs(o - ro) - rtol * np.abs(ro)).max(initial=0.0))
        fa = atol * c * (max(T.f32_per_row_excess_factor(scale, groups), F32_PER_ROW_EXCESS) if dtype == "f32" and dyn else 1.0)
        judge("fwd-excess", excess, fa, what)
        fr = BF16_D16_RAW_FWD_REL if (dtype == "bf16" and q.shape[-1] == 16 and operand_dtype is None) else frel
        judge("fwd-rel", TV._rel(o, ro), fr * c * seq_factor, what)
        no_key = (okw["attn_bias"][0] == 0).sum(axis=1) == 0
        assert (o[:, :, no_key] == 0).all() and (dq[:, :, no_key] == 0).all(), (label, "rows without a visible key must give exact zeros")
        saved = dict(o_saved=o) if operand_dtype is not None else {}
        rdq, rdk, rdv, _ = O.attention_backward(do, q, kr, vr, operand_dtype=operand_dtype, **saved, **okw)
        refs = dict(dq=rdq, dk=rdk.sum(1, keepdims=True), dv=rdv.sum(1, keepdims=True))
        for name, gg in (("dq", dq), ("dk", dk), ("dv", dv)):
            rr = refs[name]
            err = np.linalg.norm(gg - rr)
            # (the floors and float32's absolute allowance where P == 1 and the exact gradient is 0: test_gpu_fuzz.py)
            floor = (5e-2 if dtype == "f32" else 1e-3) * np.sqrt(rr.size)
            if dtype == "f32" and np.linalg.norm(rr) < floor and err <= 6e-6 * max(1.0, scale / 8.0) * np.sqrt(rr.size):
                continue
            rel = err / max(np.linalg.norm(rr), floor)
            lim = T.GRAD_TOL[dtype] * c * seq_factor
            if model_class or rel > lim:
                lim = max(lim, MODEL_SLACK * np.linalg.norm(model()[name] - rr) / max(np.linalg.norm(rr), floor))
            judge("grad-" + name, rel, lim, what)
    assert not fails, (label, fails)


def few_keys(window, causal):
    left, right = window
    right = 0 if causal else right
    return left >= 0 and right >= 0 and left + right + 1 <= 4


@pytest.mark.parametrize("name,dtype,D,B,H,Hk,N,M,left,right,kw", W.DENSE_CASES, ids=[c[0] for c in W.DENSE_CASES])
def test_window_parity(name, dtype, D, B, H, Hk, N, M, left, right, kw):
    q, k, v, do = dense_inputs(dtype, B, H, Hk, N, M, D, seed=sum(map(ord, name)), l2norm=kw.get("l2norm_qk", True))
    o, dq, dk, dv = run_local(q, k, v, do, (left, right), kw)
    G = H // Hk
    for b, hk in sorted({(B - 1, Hk - 1), (0, 0)}):
        hs = slice(hk * G, (hk + 1) * G)
        got = tuple(_np(t) for t in (o[b:b + 1, hs], dq[b:b + 1, hs], dk[b:b + 1, hk:hk + 1], dv[b:b + 1, hk:hk + 1]))
        inp = tuple(_np(t) for t in (q[b:b + 1, hs], k[b:b + 1, hk:hk + 1], v[b:b + 1, hk:hk + 1], do[b:b + 1, hs]))
        compare_slice(f"{name}[{b},{hk}]", dtype, kw, (left, right), got, inp, few_keys((left, right), kw.get("causal", False)))
    for t in (o, dq, dk, dv):
        assert torch.isfinite(t).all()


# ---- packed sequences ----------------------------------------------------------------------------------------------------------------------

def _packed_lengths(pad):
    lq, lk = list(VF.CORE_Q), list(VF.CORE_K)
    if pad is not None:
        extra = pad - len(lq)
        lq += [(7 * j) % 23 for j in range(extra)]
        lk += [(5 * j + 3) % 19 for j in range(extra)]
    return lq, lk


@pytest.mark.parametrize("name,dtype,D,H,Hk,left,right,kw,pad,mx", W.PACKED_CASES, ids=[c[0] for c in W.PACKED_CASES])
def test_window_packed_parity(name, dtype, D, H, Hk, left, right, kw, pad, mx):
    lq, lk = _packed_lengths(pad)
    q, k, v, do = TV._packed_inputs(dtype, lq, lk, H, Hk, D, seed=sum(map(ord, name)), l2norm=kw.get("l2norm_qk", True))
    qq, kk, vv = (t.detach().clone().requires_grad_() for t in (q, k, v))
    o = _F().flash_cosine_sim_attention_varlen(qq, kk, vv, TV._cu(lq), TV._cu(lk), max_seqlen_q=mx, max_seqlen_k=mx, window_size=(left, right), **kw)
    o.backward(do)
    torch.cuda.synchronize()
    cq, ck = np.concatenate([[0], np.cumsum(lq)]), np.concatenate([[0], np.cumsum(lk)])
    G = H // Hk
    for nm, t in (("o", o), ("dq", qq.grad), ("dk", kk.grad), ("dv", vv.grad)):
        assert torch.isfinite(t).all(), (name, nm)
    # the un-padded cases are compared whole: every K/V head of every sequence; the chip-filling ones on the ragged core's first and last
    # K/V head and every seventh padding sequence
    heads = range(Hk) if pad is None else sorted({0, Hk - 1})
    for s in range(len(lq)):
        sq, sk = slice(cq[s], cq[s + 1]), slice(ck[s], ck[s + 1])
        if lk[s] == 0:
            assert (o[sq] == 0).all() and (qq.grad[sq] == 0).all(), (name, s)
        if lq[s] == 0:
            assert (kk.grad[sk] == 0).all() and (vv.grad[sk] == 0).all(), (name, s)
        if lq[s] == 0 or lk[s] == 0 or (s >= len(VF.CORE_Q) and s % 7):      # the ragged core, and every seventh padding sequence
            continue
        for hk in heads:
            hs = slice(hk * G, (hk + 1) * G)
            qside = lambda t: _np(t[sq][:, hs]).transpose(1, 0, 2)[None]
            kside = lambda t: _np(t[sk][:, hk:hk + 1]).transpose(1, 0, 2)[None]
            got = (qside(o), qside(qq.grad), kside(kk.grad), kside(vv.grad))
            inp = (qside(q), kside(k), kside(v), qside(do))
            # (a short sequence on its own: the per-sequence rule of test_gpu_varlen.py::_check, 4 x the bars of the whole tensor)
            compare_slice(f"{name}[seq {s},{hk}]", dtype, kw, (left, right), got, inp, few_keys((left, right), kw.get("causal", False)) or lq[s] <= 8,
                          seq_factor=4.0 if lq[s] < 100 else 1.0)


# ---- decode --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,dtype,D,B,H,Hk,N,cap,page,lens,n_new,left,right,kw", W.DECODE_CASES, ids=[c[0] for c in W.DECODE_CASES])
def test_window_decode_parity(name, dtype, D, B, H, Hk, N, cap, page, lens, n_new, left, right, kw):
    """The policy of test_gpu_kvcache.py::_verify on the whole output: exact math on the raw inputs with the forward bars scaled by
    cases.logit_cond, and -- 16-bit types with l2norm_qk -- exact math on the 16-bit operands with the fixed bars.  16-bit types in the
    per-row-shift regime take the operand-faithful comparison only, like the dense cases above: there the two EXACT references are
    further apart than the raw bar before any kernel runs (float64 on f16 D = 16, scale 16, 8 keys, 30 seeds: raw against 16-bit operands
    differ by up to 3.8e-3 elementwise, median 1.4e-3, against the 2.5e-3 bar), so the raw comparison cannot judge a kernel."""
    q, kc, vc, kn, vn = TK._inputs(dtype, B, H, Hk, N, cap, D, n_new, seed=sum(map(ord, name)))
    l2 = kw.get("l2norm_qk", True)
    q, kc = TK._unit_normalised(q, kc, kw.get("groups", 1), l2)      # (l2norm_qk=False: the caller's inputs are unit-norm)
    if kn is not None:
        _, kn = TK._unit_normalised(q, kn, 1, l2)
    table = None
    if page:
        nb = cap // page
        perm = torch.randperm(B * nb, generator=torch.Generator().manual_seed(3)).to(torch.int32)
        table = perm.view(B, nb)
        kc, vc = (t.view(B, Hk, nb, page, D).permute(0, 2, 1, 3, 4).reshape(B * nb, Hk, page, D)[torch.argsort(perm.long())].contiguous() for t in (kc, vc))
    sl = torch.tensor(lens, dtype=torch.int32)
    with torch.no_grad():
        o = _F().flash_cosine_sim_attention_with_kvcache(q, kc, vc, kn, vn, cache_seqlens=sl, block_table=table, window_size=(left, right), **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(o).all(), name
    after = [min(n0 + n_new, cap) for n0 in lens]
    ks, vs = TK._seqs(kc, vc, after, table)
    causal = kw.get("causal", False)
    scale, groups = kw.get("scale", 8.0), kw.get("groups", 1)
    dyn = GC.dynamic_shift_regime(dtype, scale, groups, l2, False)
    cond = GC.logit_cond(dtype, scale, groups, l2)
    G = H // Hk
    passes = (None,) if dtype == "f32" or not l2 else (dtype,) if dyn else (None, dtype)
    for operand_dtype in passes:
        ref = np.zeros(q.shape)
        for b, L in enumerate(after):
            if n_new:      # the append wrote the new rows where the plain call writes them
                assert torch.equal(ks[b][:, lens[b]:L], kn[b][:, :L - lens[b]]) and torch.equal(vs[b][:, lens[b]:L], vn[b][:, :L - lens[b]])
            if L == 0:
                assert (o[b] == 0).all()
                continue
            kr, vr = (np.repeat(_np(x)[None], G, axis=1) for x in (ks[b], vs[b]))
            ref[b] = O.attention_forward_stats(_np(q[b:b + 1]), kr, vr, scale=scale, groups=groups, causal=causal, l2norm_qk=l2,
                                               attn_bias=np.repeat(band(N, L, left, right, causal), H, axis=0), eps=1e-300 if dyn else 1e-10,
                                               operand_dtype=operand_dtype)[0][0]
        c = cond if operand_dtype is None else 1.0
        if dtype == "f32" and dyn:
            c *= T.f32_per_row_excess_factor(scale, groups)
        TK._check(dtype, o, ref, f"{name}/{'raw' if operand_dtype is None else 'operands'}", c)


# ---- identities: bit for bit ---------------------------------------------------------------------------------------------------------------

IDENT = [("bf16", 64, 2, 8, 4, 300, 300), ("f16", 128, 1, 4, 4, 257, 400), ("f32", 32, 1, 2, 1, 200, 129), ("bf16", 128, 8, 32, 32, 300, 300),
         ("f16", 64, 1, 8, 8, 1024, 8192)]


@pytest.mark.parametrize("dtype,D,B,H,Hk,N,M", IDENT, ids=[f"{c[0]}_d{c[1]}_b{c[2]}h{c[3]}k{c[4]}_n{c[5]}m{c[6]}" for c in IDENT])
def test_window_identities_bit_for_bit(dtype, D, B, H, Hk, N, M):
    F = _F()
    q, k, v, do = dense_inputs(dtype, B, H, Hk, N, M, D, seed=N + M + D)

    def plain(causal):
        qq, kk, vv = (t.detach().clone().requires_grad_() for t in (q, k, v))
        o = F.flash_cosine_sim_attention(qq, kk, vv, causal=causal)
        o.backward(do)
        return o.detach(), qq.grad, kk.grad, vv.grad

    def same(a, b, what):
        for x, y, nm in zip(a, b, ("o", "dq", "dk", "dv")):
            assert torch.equal(x, y), (what, nm)

    full, causal = plain(False), plain(True)
    same(run_local(q, k, v, do, (-1, -1), dict()), full, "(-1, -1)")
    same(run_local(q, k, v, do, (-1, -1), dict(causal=True)), causal, "(-1, -1) causal")
    same(run_local(q, k, v, do, (-1, 0), dict()), causal, "(-1, 0)")
    same(run_local(q, k, v, do, (M - 1, N - 1), dict()), full, "a window that hides nothing")
    same(run_local(q, k, v, do, (M + 7, -1), dict()), full, "a window that hides nothing")
    same(run_local(q, k, v, do, (M - 1, 5), dict(causal=True)), causal, "causal caps right at 0")
    # a real window differs, and is deterministic (two runs, identical bits)
    a, b = run_local(q, k, v, do, (M // 3, 0), dict()), run_local(q, k, v, do, (M // 3, 0), dict())
    same(a, b, "two runs")
    assert not torch.equal(a[0], causal[0])


def test_window_identities_packed_and_decode():
    F = _F()
    lq, lk = [300, 0, 129, 77, 1], [250, 40, 129, 0, 300]
    q, k, v, do = TV._packed_inputs("bf16", lq, lk, 8, 2, 64, seed=21)

    def packed(window, causal):
        qq, kk, vv = (t.detach().clone().requires_grad_() for t in (q, k, v))
        kw = {} if window is None else dict(window_size=window)
        o = F.flash_cosine_sim_attention_varlen(qq, kk, vv, TV._cu(lq), TV._cu(lk), causal=causal, **kw)
        o.backward(do)
        return o.detach(), qq.grad, kk.grad, vv.grad

    for got, ref in ((packed((-1, -1), False), packed(None, False)), (packed((-1, 0), False), packed(None, True)),
                     (packed((299, 299), False), packed(None, False)), (packed((400, 3), True), packed(None, True)),
                     (packed((50, 0), True), packed((50, 0), True))):
        for x, y in zip(got, ref):
            assert torch.equal(x, y)
    assert not torch.equal(packed((50, 0), True)[0], packed(None, True)[0])
    qd, kc, vc, _, _ = TK._inputs("f16", 3, 8, 2, 5, 640, 128, 0, seed=4)
    sl = torch.tensor([640, 100, 7], dtype=torch.int32)
    with torch.no_grad():
        dec = lambda causal, **kw: F.flash_cosine_sim_attention_with_kvcache(qd, kc, vc, cache_seqlens=sl, causal=causal, **kw)
        assert torch.equal(dec(False, window_size=(-1, -1)), dec(False))
        assert torch.equal(dec(False, window_size=(-1, 0)), dec(True))
        assert torch.equal(dec(False, window_size=(639, 4)), dec(False))
        assert torch.equal(dec(True, window_size=(700, 2)), dec(True))
        assert not torch.equal(dec(True, window_size=(64, 0)), dec(True))


BIAS_ROUTE = [c for c in W.EDGE_CASES if c[6] <= c[7] and not GC.dynamic_shift_regime(c[1], c[10].get("scale", 8.0), c[10].get("groups", 1),
                                                                                      c[10].get("l2norm_qk", True), True)][::3] + \
             [c for c in W.FORM_CASES if "static" in c[0] and c[1] == "bf16" and c[6] <= c[7]][::4]


@pytest.mark.parametrize("name,dtype,D,B,H,Hk,N,M,left,right,kw", BIAS_ROUTE, ids=[c[0] for c in BIAS_ROUTE])
def test_window_matches_the_bias_route(name, dtype, D, B, H, Hk, N, M, left, right, kw):
    """the windowed call against today's route for the same problem -- the 0 / -inf band as an attn_bias -- on every (batch, head): within
    the existing bars, not bit for bit (other kernels, and for float16 another shift regime)"""
    q, k, v, do = dense_inputs(dtype, B, H, Hk, N, M, D, seed=sum(map(ord, name)), l2norm=kw.get("l2norm_qk", True))
    got = run_local(q, k, v, do, (left, right), kw)
    bias = torch.from_numpy(band(N, M, left, right, kw.get("causal", False))).to(device="cuda", dtype=DT[dtype]).expand(H, N, M).contiguous()
    qq, kk, vv = (t.detach().clone().requires_grad_() for t in (q, k, v))
    o = _F().flash_cosine_sim_attention(qq, kk, vv, attn_bias=bias, **kw)
    o.backward(do)
    cond = GC.logit_cond(dtype, kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True))
    atol, rtol, frel = T.FWD_TOL[dtype]
    ref = (o.detach(), qq.grad, kk.grad, vv.grad)
    a, r = _np(got[0]), _np(ref[0])
    excess = float((np.abs(a - r) - rtol * np.abs(r)).max(initial=0.0))
    print(f"{name}: fwd excess {excess:.3e} (bar {atol * cond:.3e}) rel {TV._rel(a, r):.3e}")
    assert T.check("window/bias-route/fwd-excess", dtype, excess, atol * cond, name)
    assert T.check("window/bias-route/fwd-rel", dtype, TV._rel(a, r), frel * cond, name)
    for nm, x, y in zip(("dq", "dk", "dv"), got[1:], ref[1:]):
        rel = TV._rel(_np(x), _np(y))
        print(f"{name}: {nm} rel {rel:.3e} (bar {T.GRAD_TOL[dtype] * cond:.3e})")
        if few_keys((left, right), kw.get("causal", False)):
            continue      # (both routes carry their own cancellation residue there: each is held against the model in test_window_parity)
        assert T.check("window/bias-route/grad", dtype, rel, T.GRAD_TOL[dtype] * cond, name), (name, nm, rel)


# ---- buffers: a NaN-filled arena with guard bands (see test_gpu_buffer_bounds.py, test_gpu_varlen.py) ---------------------------------------

def _arena_call(dtype, shape_q, shape_k, prob, window, t_of, seqs, inputs_extra=()):
    """forward + backward through the C ABI on arena buffers; returns the outputs after the guard / input / NaN checks"""
    from flash_cosine_sim_attention_amd import _lib
    lib = _lib.load()
    dt = DT[dtype]
    es = torch.empty((), dtype=dt).element_size()
    groups = prob.groups
    nq, nk = int(np.prod(shape_q)), int(np.prod(shape_k))
    rows_q, rows_k = nq // shape_q[-1], nk // shape_k[-1]
    w = _lib.Window(*window)
    sp = None if seqs is None else C.byref(seqs)
    bws_n = int(lib.fcsa_backward_window_workspace_bytes(C.byref(prob), sp, C.byref(w)))
    ar = TV.Arena((6 * nq + 7 * nk) * es + (rows_q * (1 + groups) + rows_k * groups) * 4 + bws_n + 40 * (TV.GUARD + 256))
    g = torch.Generator(device="cuda").manual_seed(nq + nk)

    def rnd(shape):
        t = ar.take(shape, dt)
        t.copy_(torch.randn(shape, device="cuda", dtype=torch.float32, generator=g).to(dt))
        return t

    q, k, v, do = rnd(shape_q), rnd(shape_k), rnd(shape_k), rnd(shape_q)
    inputs = (q, k, v, do) + tuple(inputs_extra)
    before = [t.clone() for t in inputs]
    o, dq = ar.take(shape_q, dt), ar.take(shape_q, dt)
    qn, kn = ar.take(shape_q, dt), ar.take(shape_k, dt)
    dk, dv = ar.take(shape_k, dt), ar.take(shape_k, dt)
    inv_l = ar.take((rows_q,), torch.float32)
    rq, rk = ar.take((rows_q * groups,), torch.float32), ar.take((rows_k * groups,), torch.float32)
    bws = ar.take((max(bws_n, 1),), torch.uint8)
    ptr = lambda t: t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    norm = _lib.NormState(ptr(qn), ptr(kn), ptr(rq), ptr(rk))
    fa = _lib.ForwardArgs(prob, t_of(q), t_of(k), t_of(v), t_of(o), ptr(inv_l), None, None, norm, None, 0, stream)
    _lib.check(lib.fcsa_forward_window(C.byref(fa), sp, C.byref(w)), "fcsa_forward_window")
    ba = _lib.BackwardArgs(prob, t_of(do), t_of(o), ptr(inv_l), t_of(q), t_of(k), t_of(v), None, None, norm, t_of(dq), t_of(dk), t_of(dv), None,
                           ptr(bws), bws_n, stream)
    _lib.check(lib.fcsa_backward_window(C.byref(ba), sp, C.byref(w)), "fcsa_backward_window")
    torch.cuda.synchronize()
    assert ar.guards_intact()
    for a, b in zip(inputs, before):
        assert torch.equal(a, b)
    for nm, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert not torch.isnan(t).any(), (nm, "an output row was never written, or a stream ran outside its tensor")
    return o, dq, dk, dv


@pytest.mark.parametrize("dtype,D,B,H,Hk,N,M,window,causal", [("bf16", 64, 8, 28, 28, 300, 300, (100, 0), True), ("f16", 128, 1, 4, 2, 330, 517, (64, 33), False),
                                                            ("f32", 32, 2, 2, 1, 257, 129, (31, -1), False)])
def test_window_dense_call_stays_inside_its_buffers(dtype, D, B, H, Hk, N, M, window, causal):
    from flash_cosine_sim_attention_amd import _lib
    prob = _lib.problem(DT[dtype], (B, H, Hk, N, M, D), causal, False, True, 1, 8.0)
    _arena_call(dtype, (B, H, N, D), (B, Hk, M, D), prob, window, _lib.tensor4, None)


def test_window_packed_call_stays_inside_its_buffers():
    from flash_cosine_sim_attention_amd import _lib
    lq, lk = [129, 0, 300, 1, 64, 257], [100, 7, 300, 0, 65, 300]
    ar0 = TV.Arena(1 << 12)
    cuq, cuk = TV._cu(lq).cuda(), TV._cu(lk).cuda()
    seqs = _lib.Varlen(cuq.data_ptr(), cuk.data_ptr(), sum(lq), sum(lk))
    prob = _lib.problem(torch.bfloat16, (len(lq), 4, 2, max(lq), max(lk), 64), True, False, True, 1, 8.0)
    t3 = lambda t: _lib.Tensor(t.data_ptr(), 0, t.stride(1), t.stride(0))
    _arena_call("bf16", (sum(lq), 4, 64), (sum(lk), 2, 64), prob, (70, 0), t3, seqs, inputs_extra=(cuq, cuk))
    assert ar0.guards_intact()


@pytest.mark.parametrize("page", [0, 64])
def test_window_decode_call_stays_inside_its_buffers(page):
    """the caches sit in the NaN-filled arena: a key range that starts before the cache, or a block read past the sequence's end without
    the visibility test, brings NaN into o"""
    B, H, Hk, N, cap, D = 3, 8, 2, 5, 1024, 128
    dt = torch.bfloat16
    ar = TV.Arena(4 * B * Hk * cap * D * 2 + 4 * B * H * N * D * 2 + 40 * (TV.GUARD + 256))
    g = torch.Generator(device="cuda").manual_seed(9)

    def rnd(shape):
        t = ar.take(shape, dt)
        t.copy_(torch.randn(shape, device="cuda", dtype=torch.float32, generator=g).to(dt))
        return t

    q = rnd((B, H, N, D))
    shape = (B * (cap // page), Hk, page, D) if page else (B, Hk, cap, D)
    kc, vc = rnd(shape), rnd(shape)
    table = torch.randperm(B * (cap // page), generator=torch.Generator().manual_seed(1)).to(torch.int32).view(B, -1) if page else None
    before = [t.clone() for t in (q, kc, vc)]
    sl = torch.tensor([1024, 333, 3], dtype=torch.int32)
    with torch.no_grad():
        o = _F().flash_cosine_sim_attention_with_kvcache(q, kc, vc, cache_seqlens=sl, block_table=table, causal=True, window_size=(200, 0))
    torch.cuda.synchronize()
    assert ar.guards_intact()
    for a, b in zip((q, kc, vc), before):
        assert torch.equal(a, b)
    assert torch.isfinite(o).all()


def test_window_opcheck():
    """the fake kernels of the window ops give the shapes / dtypes the binding returns, and the differentiable op registers correctly"""
    fc = torch.ops.fcsa
    _F()
    from flash_cosine_sim_attention_amd import _torch_ops
    _torch_ops.load()
    q, k, v, do = dense_inputs("bf16", 2, 4, 2, 150, 200, 64, seed=1)
    torch.library.opcheck(fc.window_forward, (q, k, v, 8.0, False, True, 1, True, 40, 3))
    torch.library.opcheck(fc.window_forward, (q, k, v, 8.0, True, True, 1, False, 40, -1), test_utils=("test_faketensor",))
    o, inv_l, qn, kn, rq, rk = fc.window_forward(q, k, v, 8.0, False, True, 1, True, 40, 3)
    torch.library.opcheck(fc.window_backward, (do, o, inv_l, q, k, v, qn, kn, rq, rk, 8.0, False, True, 1, 40, 3))
    torch.library.opcheck(fc.window_attention, (q.clone().requires_grad_(), k.clone().requires_grad_(), v.clone().requires_grad_(), 8.0, False, True, 1, 40, 3))
    lq, lk = [100, 0, 33], [90, 5, 33]
    pq, pk, pv, pdo = TV._packed_inputs("f16", lq, lk, 4, 2, 64, seed=2)
    cu_q, cu_k = TV._cu(lq).cuda(), TV._cu(lk).cuda()
    torch.library.opcheck(fc.varlen_window_forward, (pq, pk, pv, cu_q, cu_k, 100, 90, 8.0, True, True, 1, True, 20, 0))
    po, pinv, pqn, pkn, prq, prk = fc.varlen_window_forward(pq, pk, pv, cu_q, cu_k, 100, 90, 8.0, True, True, 1, True, 20, 0)
    torch.library.opcheck(fc.varlen_window_backward, (pdo, po, pinv, pq, pk, pv, cu_q, cu_k, pqn, pkn, prq, prk, 100, 90, 8.0, True, True, 1, 20, 0))
    torch.library.opcheck(fc.varlen_window_attention, (pq.clone().requires_grad_(), pk.clone().requires_grad_(), pv.clone().requires_grad_(), cu_q, cu_k,
                                                       100, 90, 8.0, True, True, 1, 20, 0))
    qd, kc, vc, kn2, vn2 = TK._inputs("bf16", 2, 4, 2, 1, 256, 64, 1, seed=3)
    sl = torch.tensor([200, 17], dtype=torch.int32, device="cuda")
    torch.library.opcheck(fc.kvcache_window_forward, (qd, kc, vc, kn2, vn2, sl, None, 256, 8.0, True, True, 1, 64, 0))
    with pytest.raises(ValueError):
        fc.window_forward(q, k, v, 8.0, False, True, 1, True, -2, 0)
