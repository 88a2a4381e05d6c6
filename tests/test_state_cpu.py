"""Attention states for training without a GPU: the two public functions and the three C-ABI symbols exist, the header mirror, the
argument checks of the new entry points (ctypes calls on fake pointers that are never dereferenced), the CPU paths against float64, and
the schemas of the `fcsa_state` ops."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import flash_cosine_sim_attention_amd as F
import lse_reference as R
import state_reference as SR
from oracle import cosine_sim_oracle as O

NEG_INF = float("-inf")
INVALID, UNSUPPORTED = -1, -2
SYMBOLS = ("fcsa_attention_lse", "fcsa_backward_state", "fcsa_merge_states_backward")

STATE_SCHEMAS = {
    "attention_state":
        "fcsa_state::attention_state(Tensor q, Tensor k, Tensor v, Tensor? cu_seqlens_q, Tensor? cu_seqlens_k, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> (Tensor, Tensor)",
    "attention_state_forward":
        "fcsa_state::attention_state_forward(Tensor q, Tensor k, Tensor v, Tensor? cu_seqlens_q, Tensor? cu_seqlens_k, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)",
    "attention_state_backward":
        "fcsa_state::attention_state_backward(Tensor? d_out, Tensor? d_lse, Tensor o, Tensor inv_l, Tensor q, Tensor k, Tensor v, Tensor? cu_seqlens_q, Tensor? cu_seqlens_k, Tensor qn, Tensor kn, Tensor rq, Tensor rk, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right) -> (Tensor, Tensor, Tensor)",
    "merge_state":
        "fcsa_state::merge_state(Tensor[] os, Tensor[] lses) -> (Tensor, Tensor)",
    "merge_state_backward":
        "fcsa_state::merge_state_backward(Tensor? d_o, Tensor? d_lse, Tensor[] os, Tensor[] lses) -> (Tensor[], Tensor[])",
}
STATE_DIFFERENTIABLE = {"attention_state", "merge_state"}


@pytest.fixture(scope="module")
def lib():
    from flash_cosine_sim_attention_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _r(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g)


def test_exports_and_header_mirror(lib):
    from flash_cosine_sim_attention_amd import _lib
    assert {"flash_cosine_sim_attention_with_lse", "merge_attention_states_with_grad"} <= set(F.__all__)
    assert callable(F.flash_cosine_sim_attention_with_lse) and callable(F.merge_attention_states_with_grad)
    assert list(inspect.signature(F.flash_cosine_sim_attention_with_lse).parameters) == [
        "q", "k", "v", "scale", "groups", "causal", "l2norm_qk", "window_size", "cu_seqlens_q", "cu_seqlens_k", "max_seqlen_q", "max_seqlen_k"]
    assert _lib.ABI_VERSION == 4 and lib.fcsa_debug(None, 0) == 4          # additive: the version stays
    for sym in SYMBOLS:
        assert sym in _lib.EXPORTS and hasattr(lib, sym)
    names = [n for n, _ in _lib.MergeBackwardArgs._fields_]
    assert names == ["dtype", "size0", "size1", "size2", "dim_head", "states", "o_in", "lse_in", "d_o", "d_lse", "d_o_in", "d_lse_in", "stream"]
    a = _lib.MergeBackwardArgs()
    assert len(a.o_in) == len(a.lse_in) == len(a.d_o_in) == len(a.d_lse_in) == 8
    # the existing structs did not grow (their full layout is pinned in test_cabi_cpu.py)
    assert C.sizeof(_lib.MergeBackwardArgs) == 24 + 8 * 32 * 4 + 32 + 32 + 8


def _bwd_args(_lib, **kw):
    a = _lib.BackwardArgs()
    a.p = _lib.problem(torch.bfloat16, (1, 2, 2, 8, 8, 64), l2norm_qk=False)
    t = _lib.Tensor(0x1000, 1024, 512, 64)
    for f in ("d_out", "o", "q", "k", "v", "dq", "dk", "dv"):
        setattr(a, f, t)
    a.inv_l = 0x2000
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_backward_state_refuses_mask_bias_and_nulls(lib):
    from flash_cosine_sim_attention_amd import _lib
    f = lib.fcsa_backward_state
    assert f(None, None, None, None) == INVALID and b"null" in lib.fcsa_last_error()
    for field in ("mask", "attn_bias", "d_bias"):
        for d_lse in (None, 0x3000):      # refused with and without an lse gradient
            assert f(C.byref(_bwd_args(_lib, **{field: 0x4000})), None, None, d_lse) == INVALID, field
            assert b"mask, attn_bias and d_bias" in lib.fcsa_last_error()
    # a valid call stops at the first thing the host can see is missing: the workspace (nothing is launched)
    assert f(C.byref(_bwd_args(_lib)), None, None, 0x3000) == -4 and b"workspace" in lib.fcsa_last_error()
    assert f(C.byref(_bwd_args(_lib, inv_l=None)), None, None, 0x3000) == INVALID and b"inv_l" in lib.fcsa_last_error()
    assert f(C.byref(_bwd_args(_lib)), None, C.byref(_lib.Window(-3, 0)), 0x3000) == INVALID and b"window" in lib.fcsa_last_error()
    seqs = _lib.Varlen(None, None, 8, 8)
    assert f(C.byref(_bwd_args(_lib)), C.byref(seqs), None, 0x3000) == INVALID and b"cu_seqlens" in lib.fcsa_last_error()
    # d_lse NULL is the existing entry point: the same refusal
    assert f(C.byref(_bwd_args(_lib)), None, None, None) == lib.fcsa_backward(C.byref(_bwd_args(_lib))) == -4


def test_attention_lse_argument_checks(lib):
    from flash_cosine_sim_attention_amd import _lib
    f = lib.fcsa_attention_lse
    p = _lib.problem(torch.bfloat16, (1, 2, 2, 8, 8, 64))
    out = _lib.LseOut(0x3000, 16, 8, 1)
    assert f(None, 0x2000, None, None, C.byref(out), None) == INVALID and b"null" in lib.fcsa_last_error()
    assert f(C.byref(p), 0x2000, None, None, None, None) == INVALID and b"null" in lib.fcsa_last_error()
    assert f(C.byref(p), None, None, None, C.byref(out), None) == INVALID and b"inv_l" in lib.fcsa_last_error()
    assert f(C.byref(p), 0x2000, None, None, C.byref(_lib.LseOut()), None) == INVALID and b"lse_out" in lib.fcsa_last_error()
    assert f(C.byref(p), 0x2000, None, C.byref(_lib.Window(0, -2)), C.byref(out), None) == INVALID and b"window" in lib.fcsa_last_error()
    assert f(C.byref(p), 0x2000, C.byref(_lib.Varlen(None, None, 8, 8)), None, C.byref(out), None) == INVALID and b"cu_seqlens" in lib.fcsa_last_error()
    bad = _lib.problem(torch.bfloat16, (1, 2, 2, 8, 8, 48))
    assert f(C.byref(bad), 0x2000, None, None, C.byref(out), None) == UNSUPPORTED
    empty = _lib.problem(torch.bfloat16, (1, 2, 2, 0, 8, 64))
    assert f(C.byref(empty), None, None, None, C.byref(_lib.LseOut()), None) == 0          # no row: nothing to do
    # fcsa_merge_states_backward
    m = lib.fcsa_merge_states_backward
    a = _lib.MergeBackwardArgs()
    a.dtype, a.size0, a.size1, a.size2, a.dim_head, a.states = 2, 2, 8, 1, 64, 9
    assert m(None) == INVALID
    assert m(C.byref(a)) == INVALID and b"states" in lib.fcsa_last_error()
    a.states, a.dim_head = 2, 6
    assert m(C.byref(a)) == UNSUPPORTED and b"dim_head" in lib.fcsa_last_error()
    a.dim_head = 64
    assert m(C.byref(a)) == INVALID and b"null" in lib.fcsa_last_error()
    a.size0 = 0
    assert m(C.byref(a)) == 0


CPU_CASES = [dict(), dict(causal=True), dict(scale=16.0, groups=2), dict(l2norm_qk=False, scale=0.5, causal=True), dict(window_size=(9, 0)),
             dict(window_size=(3, 2))]


@pytest.mark.parametrize("kw", CPU_CASES, ids=lambda kw: "_".join(f"{k}{v}" for k, v in kw.items()) or "default")
@pytest.mark.parametrize("shape", [(2, 4, 2, 5, 7, 32), (1, 2, 1, 40, 24, 16)], ids=lambda s: "x".join(map(str, s)))
def test_cpu_with_lse_against_float64(kw, shape):
    r = _r(11)
    B, H, Hk, N, M, D = shape
    q, k, v = r(B, H, N, D), r(B, Hk, M, D), r(B, Hk, M, D)
    o, lse = F.flash_cosine_sim_attention_with_lse(q, k, v, **kw)
    assert lse.shape == (B, H, N) and lse.dtype == torch.float32 and not torch.isnan(lse).any()
    okw = {a: b for a, b in kw.items() if a != "window_size"}
    win = kw.get("window_size", (-1, -1))
    for b in range(B):
        ref = R.lse_rows(q[b].double().numpy(), k[b].double().numpy(), window=win, **okw)
        got = lse[b].double().numpy()
        assert np.array_equal(np.isneginf(got), np.isneginf(ref))
        live = np.isfinite(ref)
        assert np.abs(got[live] - ref[live]).max(initial=0.0) <= 2e-5, (kw, b)
        assert (o[b].numpy()[~live] == 0).all()
    # o: the existing CPU call, and the float64 oracle (a window is a bias of 0 inside the band and -inf outside it)
    plain = (F.flash_cosine_sim_attention_local(q, k, v, win, **okw) if win != (-1, -1) else F.flash_cosine_sim_attention(q, k, v, **okw))
    assert torch.equal(o, plain)
    vis = SR.visible(N, M, kw.get("causal", False), win).numpy()
    bias = np.where(vis, 0.0, -np.inf)[None].repeat(H, 0)
    ro, _ = O.attention_forward_stats(q.double().numpy(), k.double().numpy().repeat(H // Hk, 1), v.double().numpy().repeat(H // Hk, 1),
                                      attn_bias=bias, **{a: b for a, b in okw.items() if a != "causal"})
    rows = vis.any(-1)
    assert np.abs(o.double().numpy() - ro)[:, :, rows].max(initial=0.0) <= 2e-5


def test_cpu_with_lse_packed_and_checks():
    r = _r(12)
    H, Hk, D = 4, 2, 32
    cu_q, cu_k = torch.tensor([0, 1, 34, 50], dtype=torch.int32), torch.tensor([0, 5, 5, 40], dtype=torch.int32)
    q, k, v = r(50, H, D), r(40, Hk, D), r(40, Hk, D)
    for kw in (dict(), dict(causal=True), dict(window_size=(4, 0))):
        o, lse = F.flash_cosine_sim_attention_with_lse(q, k, v, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, **kw)
        assert lse.shape == (50, H) and lse.dtype == torch.float32
        assert torch.equal(o, F.flash_cosine_sim_attention_varlen(q, k, v, cu_q, cu_k, **kw))
        assert (lse[1:34] == NEG_INF).all() and (o[1:34] == 0).all()          # a sequence without keys
        for s, (a, b, c, d) in enumerate(((0, 1, 0, 5), (34, 50, 5, 40))):
            rows = lambda t, lo, hi: t[lo:hi].transpose(0, 1).unsqueeze(0)
            o1, l1 = F.flash_cosine_sim_attention_with_lse(rows(q, a, b), rows(k, c, d), rows(v, c, d), **kw)
            assert torch.equal(rows(o, a, b), o1) and torch.equal(lse[a:b].transpose(0, 1).unsqueeze(0), l1)
    with pytest.raises(ValueError, match="together"):
        F.flash_cosine_sim_attention_with_lse(q, k, v, cu_seqlens_q=cu_q)
    with pytest.raises(ValueError, match="4-D"):
        F.flash_cosine_sim_attention_with_lse(q, k, v)
    with pytest.raises(ValueError, match="packed"):
        F.flash_cosine_sim_attention_with_lse(r(1, 2, 3, 16), r(1, 2, 3, 16), r(1, 2, 3, 16), max_seqlen_q=3)
    with pytest.raises(ValueError):
        F.flash_cosine_sim_attention_with_lse(q, k, v, cu_seqlens_q=torch.tensor([0, 1, 34, 49], dtype=torch.int32), cu_seqlens_k=cu_k)
    with pytest.raises(TypeError):
        F.flash_cosine_sim_attention_with_lse(r(1, 2, 3, 16), r(1, 2, 3, 16), r(1, 2, 3, 16), mask=None)
    with pytest.raises(RuntimeError, match="forward-only"):
        F.flash_cosine_sim_attention_with_lse(r(1, 2, 3, 16).requires_grad_(), r(1, 2, 3, 16), r(1, 2, 3, 16))


@pytest.mark.parametrize("S", [1, 2, 3, 8])
def test_cpu_merge_with_grad_against_float64_autograd(S):
    r = _r(13 + S)
    os = [r(2, 3, 5, 16).requires_grad_() for _ in range(S)]
    lses = [(3 * r(2, 3, 5)).requires_grad_() for _ in range(S)]
    with torch.no_grad():
        if S > 1:
            lses[1][0, 1] = NEG_INF          # an empty state whose o is NaN: nothing leaks, forward or backward
            os[1][0, 1] = float("nan")
        if S == 3:
            for l in lses:
                l[1, 2, 4] = NEG_INF         # a row whose every state is empty
    do, dlse = r(2, 3, 5, 16), r(2, 3, 5)
    o, lse = F.merge_attention_states_with_grad(os, lses)
    with torch.no_grad():
        o_plain, lse_plain = F.merge_attention_states([t.detach() for t in os], [t.detach() for t in lses])
    assert torch.equal(o, o_plain) and torch.equal(lse, lse_plain)
    finite = torch.isfinite(lse)
    loss = (o * do).sum() + (torch.where(finite, lse, torch.zeros_like(lse)) * dlse).sum()
    grads = torch.autograd.grad(loss, os + lses)
    ro, rl, rdo, rdl = SR.merge_reference_grads(os, lses, do, dlse)
    no, nl = R.merge_reference([t.detach().double().numpy() for t in os], [t.detach().double().numpy() for t in lses])
    assert np.abs(ro.numpy() - no).max() <= 1e-12 and np.array_equal(np.isneginf(rl.numpy()), np.isneginf(nl))      # the reference IS merge_reference's formula
    for got, ref in zip(grads, rdo + rdl):
        assert torch.isfinite(got).all()
        assert float((got.double() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
    if S > 1:
        assert (grads[1][0, 1] == 0).all() and (grads[S + 1][0, 1] == 0).all()
    with pytest.raises(ValueError, match="two steps"):
        F.merge_attention_states_with_grad(os * 9, lses * 9)
    with pytest.raises(RuntimeError, match="forward-only"):      # the old function keeps its guard
        F.merge_attention_states(os, lses)


@pytest.fixture(scope="module")
def state_ops():
    from flash_cosine_sim_attention_amd import _lib, _torch_ops
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_torch_ops.BINDING_PATH):
        _lib.build()
    _torch_ops.load()
    return torch.ops.fcsa_state


def test_state_op_set_and_schemas(state_ops):
    registered = {n.split("::", 1)[1].split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith("fcsa_state::")}
    assert registered == set(STATE_SCHEMAS)
    for name, schema in STATE_SCHEMAS.items():
        op = getattr(state_ops, name)
        assert op.overloads() == ["default"] and str(op.default._schema) == schema
    with_kernel = {n for n in STATE_SCHEMAS if torch._C._dispatch_has_kernel_for_dispatch_key("fcsa_state::" + n, "Autograd")}
    assert with_kernel == STATE_DIFFERENTIABLE
