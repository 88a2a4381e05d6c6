"""flash_cosine_sim_attention_alibi without a GPU: the function and the C entries are exported and declared (ABI version still 4, the header
states definition, sign rule, regime and the N <= M rule); the ops live in a namespace of their own with pinned schemas, fake kernels that
pass opcheck and an Autograd kernel on `attention` only; every refusal by message; the tile-ownership functions walk open-sided windowed
launches as the brute force does; and the CPU path agrees with the float64 oracle given attn_bias = band + ALiBi matrix."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import flash_cosine_sim_attention_amd as F
from flash_cosine_sim_attention_amd import _lib, _torch_ops
from test_window_cpu import band

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
alibi = F.flash_cosine_sim_attention_alibi
NS = "fcsa_alibi_train"
SYMBOLS = ("fcsa_forward_alibi", "fcsa_backward_alibi", "fcsa_forward_alibi_workspace_bytes", "fcsa_backward_alibi_workspace_bytes")
TAIL = ("Tensor? cu_seqlens_q, Tensor? cu_seqlens_k, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups, "
        "int window_left, int window_right")
SCHEMAS = {
    "forward": f"{NS}::forward(Tensor q, Tensor k, Tensor v, Tensor alibi_slopes, {TAIL}, bool need_backward) -> "
               "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)",
    "backward": f"{NS}::backward(Tensor d_out, Tensor o, Tensor inv_l, Tensor q, Tensor k, Tensor v, Tensor alibi_slopes, Tensor? cu_seqlens_q, "
                "Tensor? cu_seqlens_k, Tensor qn, Tensor kn, Tensor rq, Tensor rk, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, "
                "bool l2norm_qk, int groups, int window_left, int window_right) -> (Tensor, Tensor, Tensor)",
    "attention": f"{NS}::attention(Tensor q, Tensor k, Tensor v, Tensor alibi_slopes, {TAIL}) -> Tensor",
}


def _slopes(H):
    return torch.tensor([2.0 ** (-8.0 * (h + 1) / H) for h in range(H)], dtype=torch.float32)


def test_signature_and_export():
    params = inspect.signature(alibi).parameters
    assert list(params) == ["q", "k", "v", "alibi_slopes", "scale", "groups", "causal", "l2norm_qk", "window_size", "cu_seqlens_q", "cu_seqlens_k",
                            "max_seqlen_q", "max_seqlen_k"]
    assert params["scale"].default == 8 and params["window_size"].default == (-1, -1) and params["causal"].default is False
    assert "flash_cosine_sim_attention_alibi" in F.__all__
    doc = " ".join(alibi.__doc__.split())
    for text in ("|pos_i - j|", "pos_i = i + M - N", ">= 0", "N <= M", "captured in a graph", "no slope gradient"):
        assert text in doc, text


def test_c_entries_are_exported_declared_and_refuse_before_any_launch():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fcsa.h")).read()
    for sym in SYMBOLS:
        assert sym in _lib.EXPORTS and hasattr(lib, sym), sym
        assert re.search(r"^(int|size_t)\s+" + sym + r"\(", header, flags=re.M), sym
    assert lib.fcsa_debug(None, 0) == 4 == _lib.ABI_VERSION      # additive: the ABI version stays
    assert "#define FCSA_ABI_VERSION 4" in header
    doc = " ".join(header.replace("\n *", " ").split())
    for text in ("-slope[b, h] * |pos_i - j|", "pos_i = i + M - N", "slopes must be >= 0", "numerically undefined", "never an access out of bounds",
                 "static exponent shift of the call without slopes stays an upper bound", "N <= M rule", "q_len > k_len is refused",
                 "no existing struct changes and FCSA_ABI_VERSION stays 4"):
        assert text in doc, text
    fa, ba = _lib.ForwardArgs(), _lib.BackwardArgs()
    fa.p = ba.p = _lib.problem(torch.bfloat16, (2, 8, 2, 64, 64, 64), False, False, True, 1, 8.0)
    good = _lib.Alibi(1 << 22, 0, 1, 0)
    for call, args in ((lib.fcsa_forward_alibi, fa), (lib.fcsa_backward_alibi, ba)):
        assert call(None, None, None, None) == -1
        assert call(C.byref(args), None, None, None) == -1 and b"null slopes" in lib.fcsa_last_error()
        assert call(C.byref(args), None, None, C.byref(_lib.Alibi(None, 0, 1, 0))) == -1 and b"null slopes" in lib.fcsa_last_error()
        assert call(C.byref(args), None, None, C.byref(_lib.Alibi((1 << 22) + 2, 0, 1, 0))) == -1 and b"4-byte aligned" in lib.fcsa_last_error()
        assert call(C.byref(args), None, None, C.byref(_lib.Alibi(1 << 22, 0, 1, 9))) == -1 and b"reserved" in lib.fcsa_last_error()
        assert call(C.byref(args), None, C.byref(_lib.Window(-2, 0)), C.byref(good)) == -1 and b"window" in lib.fcsa_last_error()
    # a non-causal dense problem with q_len > k_len
    fa.p = _lib.problem(torch.bfloat16, (2, 8, 2, 65, 64, 64), False, False, True, 1, 8.0)
    assert lib.fcsa_forward_alibi(C.byref(fa), None, None, C.byref(good)) == -1 and b"q_len <= k_len" in lib.fcsa_last_error()
    # mask / attn_bias are not taken
    fa.p = _lib.problem(torch.bfloat16, (2, 8, 2, 64, 64, 64), False, False, True, 1, 8.0)
    fa.attn_bias = 1 << 23
    assert lib.fcsa_forward_alibi(C.byref(fa), None, None, C.byref(good)) == -1 and b"mask and attn_bias are not supported with alibi_slopes" in lib.fcsa_last_error()
    # the backward's workspace is the windowed plan's: no split, no group sweep
    p = _lib.problem(torch.bfloat16, (4, 8, 2, 4096, 4096, 64), True, False, True, 1, 8.0)
    assert lib.fcsa_backward_alibi_workspace_bytes(C.byref(p), None, None) == lib.fcsa_backward_window_workspace_bytes(C.byref(p), None, C.byref(_lib.Window(100, 0)))
    assert lib.fcsa_forward_alibi_workspace_bytes(C.byref(p), None, None) == 0


def test_the_ops_have_their_own_namespace_pinned_schemas_and_one_autograd_kernel():
    _torch_ops.load()
    names = {n.split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith(NS + "::")}
    assert names == {f"{NS}::{n}" for n in SCHEMAS}
    for name, schema in SCHEMAS.items():
        op = getattr(getattr(torch.ops, NS), name)
        assert op.overloads() == ["default"]
        assert str(op.default._schema) == schema
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"{NS}::{name}", "CUDA")
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"{NS}::{name}", "CPU")
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"{NS}::{name}", "Autograd") == (name == "attention")


def _fake_args(mode_tensor, packed):
    dt = dict(dtype=torch.bfloat16)
    if packed:
        q, k = mode_tensor(300, 8, 64, **dt), mode_tensor(320, 2, 64, **dt)
        cu = mode_tensor(4, dtype=torch.int32)
        return q, k, (q, k, k.clone(), mode_tensor(3, 8), cu, cu.clone(), 128, 140, 8.0, True, True, 1, 64, 0)
    q, k = mode_tensor(2, 8, 100, 64, **dt), mode_tensor(2, 2, 120, 64, **dt)
    return q, k, (q, k, k.clone(), mode_tensor(8), None, None, 0, 0, 8.0, False, True, 2, -1, -1)


@pytest.mark.parametrize("packed", [False, True])
def test_fake_kernels_give_the_shapes_and_pass_opcheck(packed):
    from torch._subclasses.fake_tensor import FakeTensorMode
    _torch_ops.load()
    ops = getattr(torch.ops, NS)
    with FakeTensorMode():
        q, k, args = _fake_args(torch.empty, packed)
        o = ops.attention(*args)
        saved = ops.forward(*args, True)
        grads = ops.backward(o, saved[0], saved[1], *args[:6], *saved[2:], *args[6:])
    rows_q, rows_k = ((8, 300), (2, 320)) if packed else ((2, 8, 100), (2, 2, 120))
    groups = args[11]
    assert o.shape == q.shape and o.dtype == q.dtype
    assert [tuple(t.shape) for t in saved] == [tuple(q.shape), rows_q, (*rows_q, 64), (*rows_k, 64), (*rows_q, groups), (*rows_k, groups)]
    assert [t.dtype for t in saved] == [q.dtype, torch.float32, q.dtype, q.dtype, torch.float32, torch.float32]
    assert [tuple(g.shape) for g in grads] == [tuple(q.shape), tuple(k.shape), tuple(k.shape)]
    meta = lambda *s, **kw: torch.empty(*s, device="meta", **kw)
    _, _, margs = _fake_args(meta, packed)
    torch.library.opcheck(ops.attention, margs, test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(ops.forward, (*margs, True), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(ops.forward, (*margs, False), test_utils=("test_schema", "test_faketensor"))
    msaved = [meta(*t.shape, dtype=t.dtype) for t in saved]
    torch.library.opcheck(ops.backward, (meta(*q.shape, dtype=q.dtype), msaved[0], msaved[1], *margs[:6], *msaved[2:], *margs[6:]),
                          test_utils=("test_schema", "test_faketensor"))


def test_refusals():
    B, H, Hk, N, M, D = 2, 4, 2, 10, 12, 16
    q, k, v = torch.randn(B, H, N, D), torch.randn(B, Hk, M, D), torch.randn(B, Hk, M, D)
    s = _slopes(H)
    with pytest.raises(TypeError, match="float32"):
        alibi(q, k, v, s.double())
    with pytest.raises(TypeError, match="float32"):
        alibi(q, k, v, [0.5] * H)
    for bad in (_slopes(H + 1), s[None].expand(B + 1, H), torch.tensor(0.5), s.reshape(H, 1)):
        with pytest.raises(ValueError, match="alibi_slopes must have shape"):
            alibi(q, k, v, bad)
    for value in (float("nan"), float("inf"), -0.25):
        t = s.clone()
        t[2] = value
        with pytest.raises(ValueError, match="finite and >= 0"):
            alibi(q, k, v, t)
    with pytest.raises(ValueError, match="no slope gradient"):
        alibi(q, k, v, s.clone().requires_grad_())
    # non-causal with N > M: dense, and any sequence of a host table
    with pytest.raises(ValueError, match="needs N <= M"):
        alibi(k.repeat(1, 2, 1, 1), q[:, :Hk], q[:, :Hk], s)
    alibi(k.repeat(1, 2, 1, 1), q[:, :Hk], q[:, :Hk], s, causal=True)      # (causal: rows without a visible key give 0)
    qp, kp = torch.randn(9, H, D), torch.randn(9, Hk, D)
    cu_q, cu_k = torch.tensor([0, 5, 9], dtype=torch.int32), torch.tensor([0, 4, 9], dtype=torch.int32)
    with pytest.raises(ValueError, match="N <= M for every sequence"):
        alibi(qp, kp, kp, s, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k)
    assert alibi(qp, kp, kp, s, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, causal=True).shape == qp.shape
    with pytest.raises(ValueError, match="given together"):
        alibi(qp, kp, kp, s, cu_seqlens_q=cu_q)
    with pytest.raises(ValueError, match="belong to packed calls"):
        alibi(q, k, v, s, max_seqlen_q=10)
    with pytest.raises(ValueError, match="4-D q, k, v"):
        alibi(q[0], k[0], v[0], s)
    with pytest.raises(ValueError, match="must start at 0"):      # the table rules of the varlen call
        alibi(qp, kp, kp, s, cu_seqlens_q=torch.tensor([1, 5, 9], dtype=torch.int32), cu_seqlens_k=cu_k, causal=True)
    with pytest.raises(RuntimeError, match="forward-only"):
        alibi(q.clone().requires_grad_(), k, v, s)
    sig = inspect.signature(alibi).parameters
    assert "mask" not in sig and "attn_bias" not in sig
    with pytest.raises(ValueError, match="alibi_slopes is on"):      # (any device but q's; a meta tensor needs no GPU)
        alibi(q, k, v, s.to("meta"))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_open_sided_windowed_launches_walk_the_brute_force_tiles(tmp_path):
    exe = str(tmp_path / "alibi_tiles_check")
    b = subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "flash_cosine_sim_attention_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "alibi_tiles_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "checks ok" in r.stdout, r.stderr[-2000:]
    assert int(r.stdout.split()[0]) > 100000


# ---- the CPU path against the float64 oracle ------------------------------------------------------------------------------------------------

def _alibi_matrix(slopes, N, M):
    i = np.arange(N)[:, None] + (M - N)
    return -np.asarray(slopes, np.float64)[:, None, None] * np.abs(i - np.arange(M)[None])[None]


@pytest.mark.parametrize("per_batch", [False, True])
@pytest.mark.parametrize("name,N,M,kw", [("causal", 40, 70, dict(causal=True)), ("noncausal", 40, 70, dict()), ("window", 50, 50, dict(window_size=(9, 2))),
                                         ("causal_window_groups", 33, 64, dict(causal=True, window_size=(20, 0), groups=2, scale=4.0)),
                                         ("causal_n_gt_m", 30, 12, dict(causal=True))])
def test_cpu_path_against_the_float64_oracle(name, N, M, kw, per_batch):
    from oracle import cosine_sim_oracle as O
    B, H, Hk, D = 2, 6, 2, 32
    g = torch.Generator().manual_seed(len(name) + N)
    q, k, v = torch.randn(B, H, N, D, generator=g), torch.randn(B, Hk, M, D, generator=g), torch.randn(B, Hk, M, D, generator=g)
    slopes = _slopes(H)
    if per_batch:
        slopes = (slopes[None] * (1 + torch.arange(B, dtype=torch.float32)[:, None])).contiguous()
    o = alibi(q, k, v, slopes, **kw)
    left, right = kw.get("window_size", (-1, -1))
    causal = kw.get("causal", False)
    npf = lambda t: t.double().numpy()
    for b in range(B):
        sl = npf(slopes if slopes.dim() == 1 else slopes[b])
        bias = band(N, M, left, right, causal) + _alibi_matrix(sl, N, M)
        kb, vb = (np.repeat(npf(t[b:b + 1]), H // Hk, axis=1) for t in (k, v))
        ref = O.attention_forward_stats(npf(q[b:b + 1]), kb, vb, scale=kw.get("scale", 8.0), groups=kw.get("groups", 1), causal=causal, l2norm_qk=True,
                                        attn_bias=bias, eps=1e-300)[0]
        # float32 arithmetic against float64: 2^-24 relative per operation over D = 32 products and <= 70 keys, logits of magnitude <= 8 + bias
        assert np.abs(npf(o[b:b + 1]) - ref).max() <= 2e-5, (name, b, np.abs(npf(o[b:b + 1]) - ref).max())
    if causal and N > M:
        assert (o[:, :, :N - M] == 0).all()


def test_cpu_packed_path_is_the_dense_path_per_sequence():
    H, Hk, D = 4, 2, 16
    lens_q, lens_k = [3, 0, 7, 5], [5, 2, 7, 9]
    g = torch.Generator().manual_seed(4)
    q, k, v = torch.randn(sum(lens_q), H, D, generator=g), torch.randn(sum(lens_k), Hk, D, generator=g), torch.randn(sum(lens_k), Hk, D, generator=g)
    cu = lambda lens: torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    slopes = (_slopes(H)[None] * torch.arange(len(lens_q), dtype=torch.float32)[:, None]).contiguous()
    o = alibi(q, k, v, slopes, causal=True, window_size=(4, 0), cu_seqlens_q=cu(lens_q), cu_seqlens_k=cu(lens_k))
    cq, ck = cu(lens_q).tolist(), cu(lens_k).tolist()
    for s, n in enumerate(lens_q):
        if n == 0:
            continue
        dense = alibi(q[cq[s]:cq[s + 1]].transpose(0, 1)[None], k[ck[s]:ck[s + 1]].transpose(0, 1)[None], v[ck[s]:ck[s + 1]].transpose(0, 1)[None],
                      slopes[s], causal=True, window_size=(4, 0))
        assert torch.equal(o[cq[s]:cq[s + 1]], dense[0].transpose(0, 1))
