"""The windowed, packed and decode calls at the sizes the README quotes speed for (tests/fullsize_feature_cases.py), where the float64
numpy oracle is too slow.  Every case is checked four ways:

  (a) random data against float64 slices (tests/fullsize_reference.py::attention_slice, pinned to the numpy oracle by
      test_fullsize_reference_cpu.py): exact math on the raw inputs with the bars scaled by cases.logit_cond, and exact math on the 16-bit
      operands with the fixed bars (in the per-row-shift regime the only comparison of the 16-bit types, as test_gpu_window.py explains).
      Forward and backward for window and packed, forward for decode (every (b, h) there).
  (b) the exact probes on the WHOLE tensor: uniform attention over sentinel values, zero pattern compared with ==, non-zero values within
      one output ulp relative (the rtol of tolerances.FWD_TOL, no absolute term), dv against its closed form by rel-L2 (GRAD_TOL).
      Decode probes keep NaN beyond each sequence's length and in pool blocks outside the table; packed probes sit in a NaN arena.
  (c) window only: the whole output and all three gradients against the existing route, the 0 / -inf band as attn_bias through
      flash_cosine_sim_attention (the rule of test_window_matches_the_bias_route: static regime, N <= M, existing bars).
  (d) identities: <dq_i, q_i> = <dk_j, k_j> = 0 (test_gpu_fullsize.py's bars), rows without a visible key give exact zeros in o and dq,
      two runs give identical bits.

Bars: tests/tolerances.py FWD_TOL / GRAD_TOL / f32_per_row_excess_factor and cases.logit_cond as they stand.  Gradients of a slice are
judged by the rule of test_gpu_window.py::compare_slice: its norm floors, float32's absolute allowance where the exact gradient is 0, a
short packed sequence on its own at 4 x the bars (below 100 rows: test_gpu_varlen.py::_check), and for slices of a handful of rows or
keys the model rule of test_gpu_fuzz.py (max(stated bar, 2 x the error of the working-precision model of the same slice)).  Every figure
is printed and logged (FCSA_TOL_LOG -> profiles/fullsize_features_margins.txt) before the case is judged.
"""
import numpy as np
import pytest
import torch

import cases as GC
import fullsize_feature_cases as FC
import fullsize_reference as FR
import test_gpu_varlen as TV
import test_gpu_window as TW
import tolerances as T

pytestmark = pytest.mark.gpu

DT = FR.DT


def _F():
    import flash_cosine_sim_attention_amd as F
    return F


def _need(gib):
    free, _ = torch.cuda.mem_get_info()
    if free < gib * 2 ** 30:
        pytest.skip(f"needs ~{gib} GiB of device memory")


def _rel(a, b):
    """rel-L2 with the floor of test_gpu_varlen.py::_rel"""
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(float(b.norm()), FR.REL_FLOOR * max(b.numel(), 1) ** 0.5))


class Judge:
    """prints and logs every figure; the case is judged at the end"""

    def __init__(self, case, dtype):
        self.case, self.dtype, self.fails = case, dtype, []

    def __call__(self, cls, measured, bar, where=""):
        print(f"{self.case} {where}: {cls} {measured:.3e} (bar {bar:.3e})")
        if not T.check("fullsize-features/" + cls, self.dtype, measured, bar, f"{self.case} {where}".strip()):
            self.fails.append((cls, where, measured, bar))

    def probe(self, cls, got, expected, where=""):
        pattern, rel = FR.probe_compare(got, expected)
        if not pattern:
            bad = ((got.double() == 0) != (expected == 0)).nonzero()
            self.fails.append((cls + "/zero-pattern", where, f"{bad.shape[0]} elements, first {bad[0].tolist()}", "exact"))
        self(cls + "/nonzero-rel", rel, T.FWD_TOL[self.dtype][1], where)

    def done(self):
        assert not self.fails, (self.case, self.fails)


def _regime(dtype, kw):
    scale, groups, l2 = kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True)
    dyn = GC.dynamic_shift_regime(dtype, scale, groups, l2, False)
    passes = (None,) if dtype == "f32" else (dtype,) if dyn else (None, dtype)
    return scale, groups, l2, dyn, GC.logit_cond(dtype, scale, groups, l2), passes


def compare_slice(j, style, where, dtype, kw, window, got, inp, factor=1.0, few_keys=False):
    """one K/V head with its G query heads against float64: got = (o, dq, dk, dv) or (o,), inp = (q, k, v, do) or (q, k, v); q-side [G, N, D],
    k-side [M, D]"""
    scale, groups, l2, dyn, cond, passes = _regime(dtype, kw)
    causal = kw.get("causal", False)
    atol, rtol, frel = T.FWD_TOL[dtype]
    q, k, v = inp[:3]
    do = inp[3] if len(inp) > 3 else None
    o = got[0]
    _, _, n = FR.visible_range(q.shape[1], k.shape[0], window, causal, device=q.device)
    assert (o[:, n == 0] == 0).all(), (j.case, where, "rows without a visible key must give exact zeros in o")
    if do is not None:
        assert (got[1][:, n == 0] == 0).all(), (j.case, where, "rows without a visible key must give exact zeros in dq")
    for opd in passes:
        c = cond if opd is None else 1.0
        what = "raw" if opd is None else "operands"
        ref = FR.attention_slice(q, k, v, do, scale=scale, groups=groups, causal=causal, window=window, l2norm_qk=l2, eps=1e-300 if dyn else 1e-10,
                                 operand_dtype=None if opd is None else DT[opd], o_saved=o if (opd is not None and do is not None) else None)
        ro = ref[0] if do is not None else ref
        excess = float(((o.double() - ro).abs() - rtol * ro.abs()).max().clamp_min(0))
        j(f"{style}/fwd-excess/{what}", excess, atol * c * (T.f32_per_row_excess_factor(scale, groups) if dtype == "f32" and dyn else 1.0), where)
        j(f"{style}/fwd-rel/{what}", _rel(o, ro), frel * c * factor, where)          # (factor: rel-L2 only, as in the rule it comes from)
        if do is not None:
            for nm, g, r in zip(("dq", "dk", "dv"), got[1:], ref[1:]):
                # the rule of test_gpu_window.py::compare_slice (floors, float32's absolute allowance where P == 1 and the exact gradient is
                # 0, and the model rule of test_gpu_fuzz.py for the few-keys class), here for slices small enough for the numpy model
                err, size = float((g.double() - r).norm()), r.numel()
                floor = FR.GRAD_FLOOR[dtype] * size ** 0.5
                if dtype == "f32" and float(r.norm()) < floor and err <= FR.F32_ZERO_GRAD_ABS * max(1.0, scale / 8.0) * size ** 0.5:
                    continue
                rel = err / max(float(r.norm()), floor)
                lim = T.GRAD_TOL[dtype] * c * factor
                if few_keys and q.numel() * k.shape[0] <= 1 << 24:
                    lim = max(lim, TW.MODEL_SLACK * _model_error(nm, dtype, kw, window, got, inp, r, opd) / max(float(r.norm()), floor))
                j(f"{style}/grad-{nm}/{what}", rel, lim, where)


def _model_error(nm, dtype, kw, window, got, inp, ref, opd):
    """||working-precision model - float64 reference|| of one gradient of a small slice (oracle.attention_backward_emulated, as
    test_gpu_window.py uses it: what a correct float32-accumulating implementation with the kernels' rounding points returns)"""
    from oracle import cosine_sim_oracle as O
    q, k, v, do = (t.detach().cpu().double().numpy() for t in inp)
    G, N, M = q.shape[0], q.shape[1], k.shape[0]
    lo, hi, _ = FR.visible_range(N, M, window, kw.get("causal", False))
    jj = np.arange(M)[None]
    bias = np.where((jj >= lo.numpy()[:, None]) & (jj <= hi.numpy()[:, None]), 0.0, -np.inf)[None].repeat(G, axis=0)
    kr, vr = (np.repeat(t[None, None], G, axis=1) for t in (k, v))
    em = O.attention_backward_emulated(do[None], q[None], kr, vr, dtype, o_saved=got[0].detach().cpu().double().numpy()[None], attn_bias=bias,
                                       scale=kw.get("scale", 8.0), groups=kw.get("groups", 1), causal=kw.get("causal", False),
                                       l2norm_qk=kw.get("l2norm_qk", True))
    model = dict(dq=em[1][0], dk=em[2][0].sum(0), dv=em[3][0].sum(0))[nm]
    return float(np.linalg.norm(model - ref.cpu().numpy()))


def tangent_identity(j, dtype, kw, q, dq, k, dk, q_zero, k_zero):
    """the gradient of a scale-invariant function is orthogonal to its argument, per l2norm group (test_gpu_fullsize.py, its bars).
    q, dq [..., N, D], k, dk [..., M, D]; q_zero [N] / k_zero [M]: the rows whose gradient is 0 in exact math by structure
    (fullsize_reference.zero_gradient_rows: a query that sees one key, a key seen only by such queries).
    bfloat16 and float32 take the identity as it is, on every row.  In float16 the kernels leave a residue of one or two SUBNORMAL steps
    on those rows (measured 6e-8 ... 2e-7 per element), whose angle to the row is arbitrary -- 0.04 ... 0.27 on the f16 cases of this
    table; the identity speaks of the direction of a gradient and those rows have none, so float16 leaves them out of it.
    In every dtype the SIZE of what the kernels leave on those rows is judged on the whole tensor, against the exact gradient 0 by the
    rule compare_slice applies to a gradient that is 0: float32's absolute allowance, rel-L2 with the norm floor for the 16-bit types."""
    scale, groups, l2, _, cond, _ = _regime(dtype, kw)
    for nm, gx, dead in (("q", dq, q_zero), ("k", dk, k_zero)):
        if bool(dead.any()):
            res = gx[..., dead, :].double()
            err, size = float(res.norm()), res.numel()
            if dtype == "f32":
                j(f"identity/zero-rows-d{nm}", err, FR.F32_ZERO_GRAD_ABS * max(1.0, scale / 8.0) * size ** 0.5)
            else:
                j(f"identity/zero-rows-d{nm}", err / (FR.GRAD_FLOOR[dtype] * size ** 0.5), T.GRAD_TOL[dtype] * cond)
    if not l2:
        return
    for nm, x, gx, dead in (("q", q, dq, q_zero), ("k", k, dk, k_zero)):
        xg = x.detach().float().reshape(*x.shape[:-1], groups, -1)
        gg = gx.float().reshape(*x.shape[:-1], groups, -1)
        ratio = (xg * gg).sum(-1).abs() / ((xg.norm(dim=-1) * gg.norm(dim=-1)) + 1e-20)
        if dtype == "f16":
            ratio = ratio.masked_fill(dead[:, None], 0.0)
        j(f"identity/tangent-{nm}", ratio.max().item(), FR.TANGENT_BAR[dtype])


def short_factor(rows):
    """a short packed sequence judged on its own: the per-sequence rule of test_gpu_varlen.py::_check, rel-L2 figures only"""
    return FR.SHORT_SEQUENCE_FACTOR if rows < FR.SHORT_SEQUENCE_ROWS else 1.0


def same_bits(a, b, what):
    for x, y, nm in zip(a, b, ("o", "dq", "dk", "dv")):
        assert torch.equal(x, y), (what, nm, "two runs must give identical bits")


# ---- window, dense call -------------------------------------------------------------------------------------------------------------------

def _dense_inputs(dtype, B, H, Hk, N, M, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32).to(DT[dtype])
    return rnd(B, H, N, D), rnd(B, Hk, M, D), rnd(B, Hk, M, D), rnd(B, H, N, D)


def _run_local(q, k, v, do, window, kw):
    q, k, v = (t.detach().requires_grad_() for t in (q, k, v))          # (no copy: strided views stay strided)
    o = _F().flash_cosine_sim_attention_local(q, k, v, window, **kw)
    o.backward(do)
    torch.cuda.synchronize()
    return o.detach(), q.grad, k.grad, v.grad


def _band_bias(N, M, window, causal, H, dtype):
    lo, hi, _ = FR.visible_range(N, M, window, causal, device="cuda")
    j = torch.arange(M, device="cuda")[None, :]
    ok = (j >= lo[:, None]) & (j <= hi[:, None])
    one = torch.where(ok, 0.0, float("-inf")).to(DT[dtype])
    del ok
    return one.expand(H, N, M).contiguous()


@pytest.mark.parametrize("name,dtype,D,B,H,Hk,N,M,left,right,kw", FC.WINDOW_CASES, ids=[c[0] for c in FC.WINDOW_CASES])
def test_window_fullsize(name, dtype, D, B, H, Hk, N, M, left, right, kw):
    _need(24)
    j = Judge(name, dtype)
    window, causal, G = (left, right), kw.get("causal", False), H // Hk
    q, k, v, do = _dense_inputs(dtype, B, H, Hk, N, M, D, seed=sum(map(ord, name)))
    got = _run_local(q, k, v, do, window, kw)
    same_bits(got, _run_local(q, k, v, do, window, kw), name)
    o, dq, dk, dv = got
    for t in got:
        assert torch.isfinite(t).all()
    # (a) float64 slices: the first, the last and one interior (batch, K/V head)
    for b, hk in sorted({(0, 0), (B - 1, Hk - 1), (B // 2, Hk // 2)}):
        hs = slice(hk * G, (hk + 1) * G)
        compare_slice(j, "window", f"[{b},{hk}]", dtype, kw, window, (o[b, hs], dq[b, hs], dk[b, hk], dv[b, hk]), (q[b, hs], k[b, hk], v[b, hk], do[b, hs]))
    # (d) identities on the whole tensors
    _, _, n = FR.visible_range(N, M, window, causal, device="cuda")
    assert (o[:, :, n == 0] == 0).all() and (dq[:, :, n == 0] == 0).all(), "rows without a visible key must give exact zeros"
    tangent_identity(j, dtype, kw, q, dq, k, dk, *FR.zero_gradient_rows(N, M, window, causal, device="cuda"))
    # (c) the bias route, whole tensors
    scale, groups, l2 = kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True)
    if N <= M and not GC.dynamic_shift_regime(dtype, scale, groups, l2, True):
        bias = _band_bias(N, M, window, causal, H, dtype)
        qq, kk, vv = (t.detach().clone().requires_grad_() for t in (q, k, v))
        ob = _F().flash_cosine_sim_attention(qq, kk, vv, attn_bias=bias, **kw)
        ob.backward(do)
        torch.cuda.synchronize()
        del bias
        cond = GC.logit_cond(dtype, scale, groups, l2)
        atol, rtol, frel = T.FWD_TOL[dtype]
        excess = float(((o.float() - ob.detach().float()).abs() - rtol * ob.detach().float().abs()).max().clamp_min(0))
        j("window/bias-route/fwd-excess", excess, atol * cond)
        j("window/bias-route/fwd-rel", _rel(o, ob.detach()), frel * cond)
        for nm, x, y in zip(("dq", "dk", "dv"), got[1:], (qq.grad, kk.grad, vv.grad)):
            j("window/bias-route/grad-" + nm, _rel(x, y), T.GRAD_TOL[dtype] * cond)
        del ob, qq, kk, vv
    del got, o, dq, dk, dv, q, k, v
    # (b) the exact probes, whole tensor
    u = FR.unit_vector(D, DT[dtype]).cuda()
    pq, pk = u.expand(B, H, N, D).contiguous(), u.expand(B, Hk, M, D).contiguous()
    pv, pos = FR.probe_v(list(range(B * Hk)), M, D, DT[dtype], device="cuda")
    pv, pos = pv.view(B, Hk, M, D), pos.view(B, Hk, D)
    o, dq, dk, dv = _run_local(pq, pk, pv, do, window, kw)
    assert torch.isfinite(dq).all() and torch.isfinite(dk).all()
    print(f"{name} probe: |dq| {dq.float().norm().item():.3e} |dk| {dk.float().norm().item():.3e} (exactly 0 in exact math)")
    worst_dv = 0.0
    for b in range(B):
        for hk in range(Hk):
            hs = slice(hk * G, (hk + 1) * G)
            j.probe("probe/window/o", o[b, hs], FR.probe_expected_o(N, M, window, causal, pos[b, hk])[None].expand(G, N, D), f"[{b},{hk}]")
            worst_dv = max(worst_dv, _rel(dv[b, hk], FR.probe_expected_dv(do[b, hs], M, window, causal)))
    j("probe/window/dv", worst_dv, T.GRAD_TOL[dtype])
    j.done()


# ---- packed -------------------------------------------------------------------------------------------------------------------------------

def _run_packed(q, k, v, do, cq, ck, mx, window, kw):
    q, k, v = (t.detach().requires_grad_() for t in (q, k, v))
    o = _F().flash_cosine_sim_attention_varlen(q, k, v, cq, ck, max_seqlen_q=mx, max_seqlen_k=mx, window_size=window, **kw)
    o.backward(do)
    torch.cuda.synchronize()
    return o.detach(), q.grad, k.grad, v.grad


def _slice_sequences(lq, lk):
    """the longest, the shortest non-empty, the first, the last, and one whose length is 1 mod 256 (where the batch has one)"""
    full = [s for s in range(len(lq)) if lq[s] and lk[s]]
    pick = {max(full, key=lambda s: lq[s]), min(full, key=lambda s: (lq[s], s)), 0, len(lq) - 1}
    pick |= set([s for s in full if lq[s] % 256 == 1 and lq[s] > 1][:1])
    return sorted(pick)


@pytest.mark.parametrize("name,dtype,D,H,Hk,lq,lk,window,kw,mx", FC.PACKED_CASES, ids=[c[0] for c in FC.PACKED_CASES])
def test_packed_fullsize(name, dtype, D, H, Hk, lq, lk, window, kw, mx):
    _need(24)
    j = Judge(name, dtype)
    lk = lq if lk is None else lk
    causal, G, S = kw.get("causal", False), H // Hk, len(lq)
    cq, ck = TV._cu(lq), TV._cu(lk)
    oq, ok_ = cq.tolist(), ck.tolist()
    q, k, v, do = TV._packed_inputs(dtype, lq, lk, H, Hk, D, seed=sum(map(ord, name)))
    got = _run_packed(q, k, v, do, cq, ck, mx, window, kw)
    same_bits(got, _run_packed(q, k, v, do, cq, ck, mx, window, kw), name)
    o, dq, dk, dv = got
    for t in got:
        assert torch.isfinite(t).all()
    for s in range(S):
        sq, sk = slice(oq[s], oq[s + 1]), slice(ok_[s], ok_[s + 1])
        if lk[s] == 0:
            assert (o[sq] == 0).all() and (dq[sq] == 0).all(), (name, s, "no key: o and dq must be zero")
        if lq[s] == 0:
            assert (dk[sk] == 0).all() and (dv[sk] == 0).all(), (name, s, "no query: dk and dv must be zero")
    for s in _slice_sequences(lq, lk):
        if lq[s] == 0 or lk[s] == 0:
            continue          # (an empty first / last sequence: judged by the zeros above)
        sq, sk = slice(oq[s], oq[s + 1]), slice(ok_[s], ok_[s + 1])
        for hk in sorted({0, Hk - 1}):
            hs = slice(hk * G, (hk + 1) * G)
            qside = lambda t: t[sq][:, hs].permute(1, 0, 2)
            kside = lambda t: t[sk][:, hk]
            compare_slice(j, "packed", f"[seq {s} ({lq[s]}x{lk[s]}),{hk}]", dtype, kw, window, (qside(o), qside(dq), kside(dk), kside(dv)),
                          (qside(q), kside(k), kside(v), qside(do)), factor=short_factor(lq[s]), few_keys=lq[s] <= 8 or lk[s] <= 4)
    dead = [FR.zero_gradient_rows(lq[s], lk[s], window, causal, device="cuda") for s in range(S)]
    tangent_identity(j, dtype, kw, q.permute(1, 0, 2), dq.permute(1, 0, 2), k.permute(1, 0, 2), dk.permute(1, 0, 2),
                     torch.cat([d[0] for d in dead]), torch.cat([d[1] for d in dead]))
    del got, o, dq, dk, dv
    # (b) the exact probes inside a NaN arena: a row read outside its span brings NaN into o or a gradient
    es = torch.empty((), dtype=DT[dtype]).element_size()
    TQ, TK = sum(lq), sum(lk)
    ar = TV.Arena((2 * TQ * H * D + 2 * TK * Hk * D) * es + 8 * (TV.GUARD + 256))
    u = FR.unit_vector(D, DT[dtype]).cuda()
    pq, pk, pv, pdo = ar.take((TQ, H, D), DT[dtype]), ar.take((TK, Hk, D), DT[dtype]), ar.take((TK, Hk, D), DT[dtype]), ar.take((TQ, H, D), DT[dtype])
    pq.copy_(u.expand(TQ, H, D))
    pk.copy_(u.expand(TK, Hk, D))
    pdo.copy_(do)
    for s in range(S):
        if lk[s]:
            pv[ok_[s]:ok_[s + 1]] = FR.probe_v([s * Hk + h for h in range(Hk)], lk[s], D, DT[dtype], device="cuda")[0].permute(1, 0, 2)
    before = [t.clone() for t in (pq, pk, pv, pdo)]
    o, dq, dk, dv = _run_packed(pq, pk, pv, pdo, cq, ck, mx, window, kw)
    assert ar.guards_intact() and all(torch.equal(a, b) for a, b in zip((pq, pk, pv, pdo), before))
    assert torch.isfinite(dq).all() and torch.isfinite(dk).all() and torch.isfinite(dv).all()
    print(f"{name} probe: |dq| {dq.float().norm().item():.3e} |dk| {dk.float().norm().item():.3e} (exactly 0 in exact math)")
    expected = torch.zeros((TQ, H, D), dtype=torch.float64, device="cuda")
    for s in range(S):
        sq, sk = slice(oq[s], oq[s + 1]), slice(ok_[s], ok_[s + 1])
        expected[sq] = FR.probe_expected_sequence(pv[sk].permute(1, 0, 2), lq[s], window, causal, G).permute(1, 0, 2)
        if lq[s] and lk[s]:      # every sequence and K/V head on its own against GRAD_TOL as it stands, short spans included
            for hk in range(Hk):
                edv = FR.probe_expected_dv(pdo[sq][:, hk * G:(hk + 1) * G].permute(1, 0, 2), lk[s], window, causal)
                j("probe/packed/dv", _rel(dv[sk][:, hk], edv), T.GRAD_TOL[dtype], f"[seq {s} ({lq[s]}x{lk[s]}),{hk}]")
        elif lk[s]:
            assert (dv[sk] == 0).all()
    j.probe("probe/packed/o", o, expected)
    j.done()


# ---- decode -------------------------------------------------------------------------------------------------------------------------------

def _paged(logical, page, spare, seed):
    """[B, Hk, cap, D] -> pool [B * nb + spare, Hk, page, D] behind a shuffled table; the spare blocks hold NaN"""
    B, Hk, cap, D = logical.shape
    nb = cap // page
    perm = torch.randperm(B * nb + spare, generator=torch.Generator().manual_seed(seed))
    table = perm[:B * nb].to(torch.int32).view(B, nb)
    pool = torch.full((B * nb + spare, Hk, page, D), float("nan"), device=logical.device, dtype=logical.dtype)
    pool[table.flatten().long().to(logical.device)] = logical.view(B, Hk, nb, page, D).permute(0, 2, 1, 3, 4).reshape(B * nb, Hk, page, D)
    return pool, table


def _decode(q, kc, vc, kn, vn, lens, table, window, kw):
    with torch.no_grad():
        o = _F().flash_cosine_sim_attention_with_kvcache(q, kc, vc, kn, vn, cache_seqlens=torch.tensor(lens, dtype=torch.int32), block_table=table,
                                                         window_size=window, **kw)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("name,dtype,D,B,H,Hk,N,cap,page,lens,n_new,window,kw", FC.DECODE_CASES, ids=[c[0] for c in FC.DECODE_CASES])
def test_decode_fullsize(name, dtype, D, B, H, Hk, N, cap, page, lens, n_new, window, kw):
    _need(16)
    j = Judge(name, dtype)
    causal, G = kw.get("causal", False), H // Hk
    after = [min(n0 + n_new, cap) for n0 in lens]
    g = torch.Generator(device="cuda").manual_seed(sum(map(ord, name)))
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32).to(DT[dtype])
    q, kc, vc = rnd(B, H, N, D), rnd(B, Hk, cap, D), rnd(B, Hk, cap, D)
    kn, vn = (rnd(B, Hk, n_new, D), rnd(B, Hk, n_new, D)) if n_new else (None, None)
    table = None
    if page:
        (kc, table), (vc, _) = _paged(kc, page, 5, 3), _paged(vc, page, 5, 3)
    # (a) random data, every (b, h) against float64
    o = _decode(q, kc, vc, kn, vn, lens, table, window, kw)
    assert torch.equal(o, _decode(q, kc, vc, kn, vn, lens, table, window, kw)), "two runs must give identical bits"
    assert torch.isfinite(o).all()
    scale, groups, l2, dyn, cond, passes = _regime(dtype, kw)
    atol, rtol, frel = T.FWD_TOL[dtype]
    refs = {opd: torch.zeros(q.shape, dtype=torch.float64, device="cuda") for opd in passes}
    for b, L in enumerate(after):
        ks, vs = FR.sequence_of_cache(kc, b, L, table), FR.sequence_of_cache(vc, b, L, table)
        if n_new:      # the append wrote the new rows where the plain call writes them
            assert torch.equal(ks[:, lens[b]:L], kn[b][:, :L - lens[b]]) and torch.equal(vs[:, lens[b]:L], vn[b][:, :L - lens[b]]), (name, b)
        if L == 0:
            assert (o[b] == 0).all()
            continue
        for hk in range(Hk):
            hs = slice(hk * G, (hk + 1) * G)
            for opd in passes:
                refs[opd][b, hs] = FR.attention_slice(q[b, hs], ks[hk], vs[hk], scale=scale, groups=groups, causal=causal, window=window, l2norm_qk=l2,
                                                      eps=1e-300 if dyn else 1e-10, operand_dtype=None if opd is None else DT[opd])
    for opd in passes:
        c, what, ro = (cond if opd is None else 1.0), ("raw" if opd is None else "operands"), refs[opd]
        j(f"decode/fwd-excess/{what}", float(((o.double() - ro).abs() - rtol * ro.abs()).max().clamp_min(0)), atol * c)
        j(f"decode/fwd-rel/{what}", _rel(o, ro), frel * c)
    del kc, vc, refs
    # (b) the exact probes: NaN beyond each sequence's length (the appended slots included, until the call writes them) and in spare blocks
    u = FR.unit_vector(D, DT[dtype]).cuda()
    pq = u.expand(B, H, N, D).contiguous()
    lk = torch.full((B, Hk, cap, D), float("nan"), device="cuda", dtype=DT[dtype])
    lv = lk.clone()
    pkn = u.expand(B, Hk, n_new, D).contiguous() if n_new else None
    pvn = torch.zeros(B, Hk, n_new, D, device="cuda", dtype=DT[dtype]) if n_new else None
    logical = []
    for b, (n0, L) in enumerate(zip(lens, after)):
        vl = FR.probe_v([b * Hk + h for h in range(Hk)], L, D, DT[dtype], device="cuda")[0]
        logical.append(vl)
        lk[b, :, :n0], lv[b, :, :n0] = u, vl[:, :n0]
        if n_new:
            pvn[b, :, :L - n0] = vl[:, n0:L]
    if page:
        (lk, _), (lv, _) = _paged(lk, page, 5, 3), _paged(lv, page, 5, 3)
    o = _decode(pq, lk, lv, pkn, pvn, lens, table, window, kw)
    # the expectation comes from the LOGICAL values, not from the cache the call wrote: the cache must hold them after the append
    expected = torch.stack([FR.probe_expected_sequence(vl, N, window, causal, G) for vl in logical])
    j.probe("probe/decode/o", o, expected)
    for b, L in enumerate(after):
        assert torch.equal(FR.sequence_of_cache(lv, b, L, table), logical[b]), (name, b, "the cache does not hold the sequence's values after the append")
        assert torch.equal(FR.sequence_of_cache(lk, b, L, table), u.expand(Hk, L, D)), (name, b, "the cache does not hold the sequence's keys after the append")
    for b, (n0, L) in enumerate(zip(lens, after)):      # untouched beyond the appended rows: still NaN
        tail = FR.sequence_of_cache(lv, b, cap, table)[:, L:]
        assert torch.isnan(tail).all(), (name, b, "a cache slot beyond the sequence was written")
    j.done()
