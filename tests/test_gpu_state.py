"""Attention states for training on the GPU: flash_cosine_sim_attention_with_lse (dense, local, packed) and
merge_attention_states_with_grad.

Reference: tests/state_reference.py, float64 torch autograd on the CPU of loss = <o, do> + <lse, dlse> over the plain composite on the same
inputs -- for the 16-bit types on the operands the kernels are fed (operand-faithful, as in the parity tests), for float32 on the raw
inputs; the lse is also held to lse_reference.derived_lse_bound against float64 on the RAW inputs.  Bars: tests/tolerances_state.py.
Exact identities carry no tolerance: o and -- without an lse gradient -- dq, dk, dv are the existing call's bits; do = 0 gives dv = 0;
rows without a visible key have lse = -inf and take no gradient whatever their dlse holds.
Where the 16-bit forward's row sum of ROUNDED P~ cannot meet the derived bound (l2norm_qk off, or |scale| groups < 1/2: the bound is then
below one unit roundoff of the type) the binding reads the lse off a float32 forward; the "lse-from-float32-pass" cases are those.
Every case's id names the dQ / dK/dV forms it launches at 256 CUs (recorded with tests/native/launch_recorder.cpp:
bwd_dq<type, D, waves, bias, tiles per stage, two-wave tile, key mask, wave-half key split>).  Chip-filling cases compare one batch slice."""
import numpy as np
import pytest
import torch

import lse_reference as R
import state_reference as SR
import tolerances as T
import tolerances_state as TS

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
NEG_INF = float("-inf")


def _F():
    import flash_cosine_sim_attention_amd as F
    return F


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _inputs(dtype, B, H, Hk, N, M, D, seed, l2norm=True):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32)
    q, k, v, do, dlse = rnd(B, H, N, D), rnd(B, Hk, M, D), rnd(B, Hk, M, D), rnd(B, H, N, D), rnd(B, H, N)
    if not l2norm:
        q, k = torch.nn.functional.normalize(q, dim=-1), torch.nn.functional.normalize(k, dim=-1)
    return tuple(t.to(DT[dtype]) for t in (q, k, v, do)) + (dlse,)


def _run(fn, q, k, v, do, dlse):
    """fn(q, k, v) -> o or (o, lse); backward of <o, do> (+ <lse, dlse>); (o, lse or None, dq, dk, dv)"""
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    out = fn(q, k, v)
    o, lse = out if isinstance(out, tuple) else (out, None)
    if dlse is None:
        o.backward(do)
    else:
        torch.autograd.backward([o, lse], [do, dlse])
    torch.cuda.synchronize()
    return o.detach(), None if lse is None else lse.detach(), q.grad, k.grad, v.grad


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _judge(fails, label, dtype, cls, measured, bar):
    print(f"{label}: {cls} {measured:.3e} (bar {bar:.3e})")
    if not T.check("state/" + cls, dtype, measured, bar, label):
        fails.append((cls, measured, bar))


def _exact_identities(label, plain, state, q, k, v, do, dlse, lse_mask_of):
    """the tolerance-free part, shared by the dense and the packed cases; returns the state call's (o, lse, dq, dk, dv) with dlse"""
    o0, _, dq0, dk0, dv0 = _run(plain, q, k, v, do, None)
    o1, lse1, dq1, dk1, dv1 = _run(state, q, k, v, do, None)                       # dlse omitted
    assert _bits_equal(o1, o0), (label, "o must be the existing call's o")
    assert _bits_equal(dq1, dq0) and _bits_equal(dk1, dk0) and _bits_equal(dv1, dv0), (label, "no dlse: the existing call's gradients")
    _, _, dq2, dk2, dv2 = _run(state, q, k, v, do, torch.zeros_like(dlse))          # dlse zero
    assert _bits_equal(dq2, dq0) and _bits_equal(dk2, dk0) and _bits_equal(dv2, dv0), (label, "dlse = 0: the existing call's gradients")
    _, _, _, _, dv3 = _run(state, q, k, v, torch.zeros_like(do), dlse)              # do = 0: dv = P^T do
    assert (dv3 == 0).all(), (label, "do = 0 must give dv = 0 exactly")
    got = _run(state, q, k, v, do, dlse)
    assert _bits_equal(got[0], o0)
    empty = lse_mask_of(lse1)
    assert torch.equal(lse1 == NEG_INF, empty) and not torch.isnan(lse1).any(), (label, "lse = -inf exactly on the rows without a visible key")
    if empty.any():
        huge = torch.where(empty, torch.full_like(dlse, 1e30), dlse)
        again = _run(state, q, k, v, do, huge)
        assert all(_bits_equal(a, b) for a, b in zip(again[2:], got[2:])), (label, "an empty row's dlse must not move a gradient bit")
        assert all(torch.isfinite(t).all() for t in again[2:])
    return got


# (id, dtype, (B, H, Hk, N, M, D), keywords, split-form factor applies, batches the reference runs on)
DENSE = [
    ("n5_m7_dq-b64w8-ksplit-km", "bf16", (1, 2, 2, 5, 7, 64), dict(), False, None),
    ("n45_m77_dq-h64w8-ksplit-km", "f16", (2, 3, 3, 45, 77, 64), dict(), False, None),
    ("n45_m77_causal_dq-h64w8-ksplit", "f16", (2, 3, 3, 45, 77, 64), dict(causal=True), False, None),
    ("n40_m24_causal_16-empty-rows_dq-b64w8-ksplit", "bf16", (1, 2, 2, 40, 24, 64), dict(causal=True), False, None),
    ("n512_m300_causal_dq-b64w8-ksplit_dkv-w8", "bf16", (1, 1, 1, 512, 300, 64), dict(causal=True), False, None),
    ("chip_n256_m1000_dq-h64w8-sub4-km", "f16", (28, 8, 8, 256, 1000, 64), dict(), False, (0, 27)),
    ("chip_n256_causal_dq-b64w8-sub4_dkv-w8", "bf16", (32, 8, 8, 256, 256, 64), dict(causal=True), False, (31,)),
    ("d128_causal_dq-b128w8-ksplit", "bf16", (1, 2, 2, 200, 300, 128), dict(causal=True), False, None),
    ("d128_dq-h128w4-km", "f16", (1, 2, 2, 200, 300, 128), dict(), False, None),
    ("f32_d64_causal_dq-f64w4", "f32", (1, 2, 2, 100, 130, 64), dict(causal=True), False, None),
    ("f32_d128_dq-f128w4-km", "f32", (1, 2, 2, 100, 130, 128), dict(), False, None),
    ("split-dq-keys-x8_n128_m4096_dq-b64w4-km", "bf16", (1, 2, 2, 128, 4096, 64), dict(), True, None),
    ("split-dkv-queries-x8_n4096_m128_dq-b64w8-ksplit-km", "bf16", (1, 2, 2, 4096, 128, 64), dict(), True, None),
    ("h4_hk2_dq-b64w8-ksplit-km", "bf16", (2, 4, 2, 100, 130, 64), dict(), False, None),
    ("h4_hk1_causal_dq-b64w8-ksplit", "bf16", (2, 4, 1, 100, 130, 64), dict(causal=True), False, None),
    ("d16_causal_dq-h16w8-ksplit", "f16", (1, 2, 2, 70, 90, 16), dict(causal=True), False, None),
    ("d96_dq-b96w4-km", "bf16", (1, 2, 2, 70, 90, 96), dict(), False, None),
    ("no-l2norm_dq-h64w8-ksplit-km", "f16", (1, 2, 2, 70, 90, 64), dict(l2norm_qk=False), False, None),
    ("scale0.25_f16_lse-from-float32-pass", "f16", (1, 2, 2, 70, 90, 64), dict(scale=0.25), False, None),
    ("no-l2norm_bf16_causal_lse-from-float32-pass", "bf16", (1, 2, 1, 70, 90, 64), dict(l2norm_qk=False, causal=True), False, None),
    ("per-row-shift_f16_scale16_causal", "f16", (1, 2, 2, 70, 90, 64), dict(scale=16.0, causal=True), False, None),
    ("per-row-shift_bf16_scale80", "bf16", (1, 2, 2, 70, 90, 64), dict(scale=80.0), False, None),
    ("window16-8_dq-win", "bf16", (1, 2, 2, 100, 130, 64), dict(window_size=(16, 8)), False, None),
    ("window20-0_causal_n-gt-m_dq-win", "f16", (2, 4, 2, 130, 100, 64), dict(window_size=(20, 0), causal=True), False, None),
    ("window5-2_f32_d128_hk1_dq-win", "f32", (1, 2, 1, 45, 77, 128), dict(window_size=(5, 2)), False, None),
]


def _compare(label, dtype, kw, split, got, ref_raw, ref_ops):
    """got / refs = (o, lse, dq, dk, dv); ref_ops: the operand-faithful reference (float32: the raw one)"""
    fails = []
    scale, groups, l2 = kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True)
    lse = got[1].detach().cpu().double()
    live = torch.isfinite(ref_raw[1])
    assert torch.equal(torch.isfinite(lse), live), label
    _judge(fails, label, dtype, "lse-raw", float((lse - ref_raw[1])[live].abs().max()) if live.any() else 0.0,
           R.derived_lse_bound(dtype, scale, groups, l2))
    _judge(fails, label, dtype, "lse-operands", float((lse - ref_ops[1])[live].abs().max()) if live.any() else 0.0, TS.STATE_LSE_TOL[dtype])
    bar = TS.STATE_SPLIT_GRAD_TOL[dtype] if split else TS.STATE_GRAD_TOL[dtype]
    for name, g, r in zip(("dq", "dk", "dv"), got[2:], ref_ops[2:]):
        assert torch.isfinite(g).all(), (label, name)
        _judge(fails, label, dtype, "grad-" + name + ("-split" if split else ""), _rel(g, r), bar)
    assert not fails, (label, fails)


@pytest.mark.parametrize("case", DENSE, ids=[c[0] for c in DENSE])
def test_dense_and_local_state(case):
    label, dtype, (B, H, Hk, N, M, D), kw, split, ref_batches = case
    F = _F()
    q, k, v, do, dlse = _inputs(dtype, B, H, Hk, N, M, D, seed=len(label), l2norm=kw.get("l2norm_qk", True))
    win = kw.get("window_size", (-1, -1))
    okw = {a: b for a, b in kw.items() if a != "window_size"}
    plain = (lambda q, k, v: F.flash_cosine_sim_attention_local(q, k, v, win, **okw)) if win != (-1, -1) else \
            (lambda q, k, v: F.flash_cosine_sim_attention(q, k, v, **okw))
    state = lambda q, k, v: F.flash_cosine_sim_attention_with_lse(q, k, v, **kw)
    vis = SR.visible(N, M, kw.get("causal", False), win)
    empty_rows = (~vis.any(-1)).cuda()
    got = _exact_identities(label, plain, state, q, k, v, do, dlse, lambda lse: empty_rows.expand_as(lse))
    assert got[1].shape == (B, H, N) and got[1].dtype == torch.float32
    assert (got[0][:, :, empty_rows] == 0).all() and (got[2][:, :, empty_rows] == 0).all()
    rkw = dict(scale=kw.get("scale", 8.0), groups=kw.get("groups", 1), causal=kw.get("causal", False), l2norm_qk=kw.get("l2norm_qk", True), window=win)
    for b in (range(B) if ref_batches is None else ref_batches):
        sl = slice(b, b + 1)
        raw = SR.reference(q[sl], k[sl], v[sl], do[sl], dlse[sl], **rkw)
        ops = raw if dtype == "f32" else SR.reference(q[sl], k[sl], v[sl], do[sl], dlse[sl], operand_dtype=dtype, **rkw)
        _compare(f"{label}/b{b}", dtype, kw, split, tuple(t[sl] for t in got), raw, ops)


PACKED_Q, PACKED_K = [0, 1, 33, 130], [5, 0, 33, 64]


@pytest.mark.parametrize("window", [(-1, -1), (16, 0)], ids=["full", "window16-0"])
@pytest.mark.parametrize("causal", [False, True], ids=["", "causal"])
@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f32", 32)], ids=["bf16-d64", "f32-d32"])
def test_packed_state(dtype, D, causal, window):
    label = f"packed_{dtype}_d{D}_{'causal' if causal else 'full'}_{window}"
    F = _F()
    H, Hk = 4, 2
    cu_q = torch.tensor(np.concatenate([[0], np.cumsum(PACKED_Q)]), dtype=torch.int32)
    cu_k = torch.tensor(np.concatenate([[0], np.cumsum(PACKED_K)]), dtype=torch.int32)
    TQ, TK = int(cu_q[-1]), int(cu_k[-1])
    g = torch.Generator(device="cuda").manual_seed(7)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32)
    q, k, v, do = (t.to(DT[dtype]) for t in (rnd(TQ, H, D), rnd(TK, Hk, D), rnd(TK, Hk, D), rnd(TQ, H, D)))
    dlse = rnd(H, TQ).t()                                   # [total_q, H] with strides of its own: the binding brings it into inv_l's layout
    kw = dict(causal=causal, window_size=window)
    plain = lambda q, k, v: F.flash_cosine_sim_attention_varlen(q, k, v, cu_q, cu_k, **kw)
    state = lambda q, k, v: F.flash_cosine_sim_attention_with_lse(q, k, v, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, **kw)
    empty = torch.zeros(TQ, dtype=torch.bool)
    for s in range(len(PACKED_Q)):
        vis = SR.visible(PACKED_Q[s], PACKED_K[s], causal, window)
        empty[int(cu_q[s]):int(cu_q[s + 1])] = ~vis.any(-1) if PACKED_K[s] else True
    empty = empty.cuda()
    got = _exact_identities(label, plain, state, q, k, v, do, dlse, lambda lse: empty[:, None].expand_as(lse))
    assert got[1].shape == (TQ, H) and got[1].dtype == torch.float32
    rkw = dict(causal=causal, window=window)
    cq, ck = cu_q.tolist(), cu_k.tolist()
    raw = SR.reference_packed(q.cpu(), k.cpu(), v.cpu(), do.cpu(), dlse.cpu(), cq, ck, **rkw)
    ops = raw if dtype == "f32" else SR.reference_packed(q.cpu(), k.cpu(), v.cpu(), do.cpu(), dlse.cpu(), cq, ck, operand_dtype=dtype, **rkw)
    _compare(label, dtype, dict(), False, got, raw, ops)


# ---- the differentiable merge ------------------------------------------------------------------------------------------------------------

def _states(dtype, shape, S, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32)
    os = [rnd(*shape).to(DT[dtype]) for _ in range(S)]
    lses = [3 * rnd(*shape[:-1]) for _ in range(S)]
    return os, lses, rnd(*shape).to(DT[dtype]), rnd(*shape[:-1])


@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("dtype,shape", [("bf16", (2, 3, 37, 64)), ("f16", (2, 2, 5, 96)), ("f32", (1, 2, 33, 16)), ("bf16", (50, 4, 128)),
                                         ("f32", (3, 2, 7, 96))], ids=["bf16-d64", "f16-d96", "f32-d16", "bf16-packed-d128", "f32-d96"])
def test_merge_backward_against_float64(dtype, shape, S):
    label = f"merge_{dtype}_{shape}_S{S}"
    F = _F()
    os, lses, do, dlse = _states(dtype, shape, S, seed=S)
    nan_state = S > 1
    if nan_state:                                           # state 1 is empty on a block of rows and holds NaN there
        lses[1][0] = NEG_INF
        os[1][0] = float("nan")
    if S == 3:                                              # ... and one row has every state empty
        for l in lses:
            l[-1, -1] = NEG_INF
    # through strided views: the states as slices of one buffer
    buf = torch.stack(os, dim=-2)                           # [..., S, D]
    views = [buf.select(-2, s) for s in range(S)]
    with torch.no_grad():
        o0, lse0 = F.merge_attention_states(views, lses)
    ins = [t.detach().clone().requires_grad_() for t in os] + [t.detach().clone().requires_grad_() for t in lses]
    o, lse = F.merge_attention_states_with_grad(ins[:S], ins[S:])
    assert _bits_equal(o, o0) and _bits_equal(lse, lse0), (label, "the forward kernel, bit for bit")
    finite = torch.isfinite(lse)
    torch.autograd.backward([o, torch.where(finite, lse, torch.zeros_like(lse))], [do, dlse])
    torch.cuda.synchronize()
    _, _, rdo, rdl = SR.merge_reference_grads(os, lses, do, dlse)
    u = R.ULP[dtype]
    fails = []
    gmax = float(do.float().abs().max())
    for s in range(S):
        gd, gl = ins[s].grad, ins[S + s].grad
        assert torch.isfinite(gd).all() and torch.isfinite(gl).all(), (label, s)
        err = (gd.cpu().double() - rdo[s]).abs() - u * rdo[s].abs()
        _judge(fails, label, dtype, "merge-do-excess", float(err.max()) / gmax, TS.MERGE_DO_ATOL)
        _judge(fails, label, dtype, "merge-dlse", float((gl.cpu().double() - rdl[s]).abs().max()) / max(1.0, float(rdl[s].abs().max())), TS.MERGE_DLSE_TOL)
    if nan_state:
        assert (ins[1].grad[0] == 0).all() and (ins[S + 1].grad[0] == 0).all(), (label, "a state of weight 0 takes exactly zero gradients")
    if S == 3:
        assert all((t.grad[-1, -1] == 0).all() for t in ins), (label, "every state empty: everything 0")
    # only one of the two results used: the other gradient is absent, not zeros
    ins2 = [t.detach().clone().requires_grad_() for t in os] + [t.detach().clone().requires_grad_() for t in lses]
    o2, lse2 = F.merge_attention_states_with_grad(ins2[:S], ins2[S:])
    o2.backward(do)
    ins3 = [t.detach().clone().requires_grad_() for t in os] + [t.detach().clone().requires_grad_() for t in lses]
    o3, lse3 = F.merge_attention_states_with_grad(ins3[:S], ins3[S:])
    torch.autograd.backward([o3, torch.where(finite, lse3, torch.zeros_like(lse3))], [do, torch.zeros_like(dlse)])
    assert all(_bits_equal(a.grad, b.grad) for a, b in zip(ins2, ins3)), (label, "dlse absent == dlse zero")
    assert not fails, (label, fails)


# ---- composition: one attention over key chunks, and the causal ring schedule ---------------------------------------------------------------

def _chunked(F, q, k, v, edges, kw):
    """non-causal: the states of the key chunks [edges[i], edges[i + 1]) merged"""
    states = [F.flash_cosine_sim_attention_with_lse(q, k[:, :, lo:hi], v[:, :, lo:hi], **kw) for lo, hi in zip(edges[:-1], edges[1:])]
    return F.merge_attention_states_with_grad([s[0] for s in states], [s[1] for s in states])


def _ring(F, q, k, v, chunk, kw):
    """the causal ring schedule: the N queries are the last N of the M positions, both cut into chunks of `chunk`; key chunk j of query chunk
    i (global chunk index c = i + (M - N) / chunk) runs non-causal for j < c, causal for j == c, and is skipped for j > c"""
    N, M = q.shape[2], k.shape[2]
    off = (M - N) // chunk
    outs, lses = [], []
    for i in range(N // chunk):
        qi = q[:, :, i * chunk:(i + 1) * chunk]
        states = [F.flash_cosine_sim_attention_with_lse(qi, k[:, :, j * chunk:(j + 1) * chunk], v[:, :, j * chunk:(j + 1) * chunk],
                                                        causal=(j == i + off), **kw) for j in range(i + off + 1)]
        o, lse = F.merge_attention_states_with_grad([s[0] for s in states], [s[1] for s in states])
        outs.append(o)
        lses.append(lse)
    return torch.cat(outs, dim=2), torch.cat(lses, dim=2)


COMPOSED = [
    ("two-chunks", "bf16", (2, 4, 2, 70, 150, 64), False, lambda F, kw: (lambda q, k, v: _chunked(F, q, k, v, [0, 77, 150], kw))),
    ("three-chunks", "f16", (2, 4, 2, 70, 150, 64), False, lambda F, kw: (lambda q, k, v: _chunked(F, q, k, v, [0, 32, 77, 150], kw))),
    ("three-chunks", "f32", (1, 2, 2, 70, 150, 32), False, lambda F, kw: (lambda q, k, v: _chunked(F, q, k, v, [0, 32, 77, 150], kw))),
    ("ring-96-96", "bf16", (1, 2, 2, 96, 96, 64), True, lambda F, kw: (lambda q, k, v: _ring(F, q, k, v, 32, kw))),
    ("ring-96-96", "f32", (1, 2, 2, 96, 96, 64), True, lambda F, kw: (lambda q, k, v: _ring(F, q, k, v, 32, kw))),
    ("ring-64-128", "f16", (1, 4, 2, 64, 128, 64), True, lambda F, kw: (lambda q, k, v: _ring(F, q, k, v, 32, kw))),
]


@pytest.mark.parametrize("case", COMPOSED, ids=[f"{c[0]}_{c[1]}" for c in COMPOSED])
def test_composed_against_single_call(case):
    name, dtype, (B, H, Hk, N, M, D), causal, make = case
    label = f"composed_{name}_{dtype}"
    F = _F()
    q, k, v, do, dlse = _inputs(dtype, B, H, Hk, N, M, D, seed=11)
    single = _run(lambda q, k, v: F.flash_cosine_sim_attention_with_lse(q, k, v, causal=causal), q, k, v, do, dlse)
    comp = _run(make(F, dict()), q, k, v, do, dlse)
    ref = SR.reference(q, k, v, do, dlse, causal=causal, operand_dtype=None if dtype == "f32" else dtype)
    fails = []
    for what, c, s, r in zip(("o", "lse", "dq", "dk", "dv"), comp, single, ref):
        ec, es = _rel(c, r), _rel(s, r)
        print(f"{label}: {what} composed {ec:.3e} single {es:.3e}")
        _judge(fails, label, dtype, "composed-over-single-" + what, ec / es, TS.COMPOSED_FACTOR)
    assert not fails, (label, fails)


# ---- opcheck and gradcheck ------------------------------------------------------------------------------------------------------------

def test_state_opcheck():
    _F()
    from flash_cosine_sim_attention_amd import _torch_ops
    _torch_ops.load()
    st = torch.ops.fcsa_state
    q, k, v, do, dlse = _inputs("bf16", 2, 4, 2, 50, 70, 64, seed=1)
    rg = lambda t: t.clone().requires_grad_()
    torch.library.opcheck(st.attention_state_forward, (q, k, v, None, None, 0, 0, 8.0, True, True, 1, -1, -1))
    torch.library.opcheck(st.attention_state_forward, (q, k, v, None, None, 0, 0, 8.0, False, True, 1, 10, 3))
    o, lse, inv_l, qn, kn, rq, rk = st.attention_state_forward(q, k, v, None, None, 0, 0, 8.0, False, True, 1, 10, 3)
    torch.library.opcheck(st.attention_state_backward, (do, dlse, o, inv_l, q, k, v, None, None, qn, kn, rq, rk, 0, 0, 8.0, False, True, 1, 10, 3))
    torch.library.opcheck(st.attention_state_backward, (do, None, o, inv_l, q, k, v, None, None, qn, kn, rq, rk, 0, 0, 8.0, False, True, 1, 10, 3))
    torch.library.opcheck(st.attention_state, (rg(q), rg(k), rg(v), None, None, 0, 0, 8.0, True, True, 1, -1, -1))
    cu_q = torch.tensor([0, 0, 1, 34, 50], dtype=torch.int32, device="cuda")
    cu_k = torch.tensor([0, 5, 5, 38, 70], dtype=torch.int32, device="cuda")
    pq, pk, pv = q[0].transpose(0, 1).contiguous(), k[0].transpose(0, 1).contiguous(), v[0].transpose(0, 1).contiguous()
    torch.library.opcheck(st.attention_state_forward, (pq, pk, pv, cu_q, cu_k, 33, 33, 8.0, True, True, 1, -1, -1))
    torch.library.opcheck(st.attention_state, (rg(pq), rg(pk), rg(pv), cu_q, cu_k, 33, 33, 8.0, False, True, 1, 16, 0))
    os, lses, mdo, mdl = _states("bf16", (2, 4, 3, 32), 3, seed=3)
    torch.library.opcheck(st.merge_state, ([rg(t) for t in os], [rg(t) for t in lses]))
    torch.library.opcheck(st.merge_state_backward, (mdo, mdl, os, lses))
    torch.library.opcheck(st.merge_state_backward, (mdo.flatten(0, 1), None, [t.flatten(0, 1) for t in os], [t.flatten(0, 1) for t in lses]))


def test_gradcheck_float32():
    """torch.autograd.gradcheck in float32 on (1, 1, 5, 7, D 16), both functions: central differences with eps = 1e-2 of float32 kernels
    whose outputs are O(1) carry u / eps ~ 6e-6 of rounding noise plus the O(eps^2) truncation of a softmax at scale 8; the tolerances of
    tolerances_state.GRADCHECK (atol = rtol = 2e-3) are what that leaves room for."""
    F = _F()
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32).requires_grad_()
    q, k, v = rnd(1, 1, 5, 16), rnd(1, 1, 7, 16), rnd(1, 1, 7, 16)
    for kw in (dict(scale=2.0), dict(scale=2.0, causal=True), dict(scale=2.0, l2norm_qk=False)):
        assert torch.autograd.gradcheck(lambda q, k, v: F.flash_cosine_sim_attention_with_lse(q, k, v, **kw), (q, k, v), nondet_tol=0.0,
                                        **TS.GRADCHECK), kw
    os = [rnd(1, 1, 5, 16) for _ in range(3)]
    lses = [rnd(1, 1, 5) for _ in range(3)]
    assert torch.autograd.gradcheck(lambda *t: F.merge_attention_states_with_grad(t[:3], t[3:]), (*os, *lses), nondet_tol=0.0, **TS.GRADCHECK)
