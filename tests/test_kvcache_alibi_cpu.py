"""flash_cosine_sim_attention_alibi_with_kvcache without a GPU: its signature is the step call's plus alibi_slopes, last, and without slopes it
is the step call; bad slopes are refused; the op lives in a namespace of its own with a pinned schema, a fake kernel and no Autograd
kernel; the C entry is exported, declared and refuses NULL, misaligned and reserved arguments before any launch; and the CPU path agrees
with the float64 oracle given attn_bias = band + ALiBi matrix (causal, non-causal and windowed)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import flash_cosine_sim_attention_amd as F
from flash_cosine_sim_attention_amd import _lib, _torch_ops
from test_kvcache_prefill_cpu import _problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
alibi = F.flash_cosine_sim_attention_alibi_with_kvcache
step = F.flash_cosine_sim_attention_step_with_kvcache
NAME = "flash_cosine_sim_attention_alibi_with_kvcache"

SCHEMA = ("fcsa_alibi::kvcache_alibi_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor cu_seqlens_q, Tensor alibi_slopes, "
          "Tensor? k_new, Tensor? v_new, Tensor? cache_seqlens, Tensor? block_table, Tensor? k_scale, Tensor? v_scale, int max_seqlen_q, "
          "int max_seqlen_k, float scale, bool causal, bool l2norm_qk, int groups, int window_left, int window_right, int chunk_rows, "
          "int max_decode_tokens, bool no_decode, bool no_chunk) -> (Tensor, Tensor)")
COUNTS, CACHED = [1, 0, 5, 40], [0, 17, 30, 3]
H, HK, D = 6, 2, 64


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _slopes(heads=H):
    return torch.tensor([2.0 ** (-8.0 * (h + 1) / heads) for h in range(heads)], dtype=torch.float32)


def test_signature_is_the_step_calls_plus_alibi_slopes():
    mine, theirs = inspect.signature(alibi).parameters, inspect.signature(step).parameters
    assert list(mine) == list(theirs) + ["alibi_slopes"]
    assert all(mine[n] == theirs[n] for n in theirs)
    assert mine["alibi_slopes"].default is None
    assert NAME in F.__all__
    doc = " ".join(alibi.__doc__.split())
    assert "flash_cosine_sim_attention_step_with_kvcache" in doc and "|pos_i - j|" in doc and "per-row-shift regime" in doc


@pytest.mark.parametrize("page,append,causal", [(0, True, True), (16, False, False)])
def test_without_slopes_it_is_the_step_call(page, append, causal):
    q, kc, vc, cu, kn, vn, lens, table = _problem(torch.bfloat16, D, H, HK, COUNTS, CACHED, 64, page, 3)
    if not append:
        kn = vn = None
    outs = []
    for fn in (alibi, step):
        k2, v2 = kc.clone(), vc.clone()
        o, lse = fn(q, k2, v2, cu, kn, vn, cache_seqlens=lens, block_table=table, causal=causal, return_lse=True, chunk_rows=7)
        outs.append((o, lse, k2, v2))
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b))


def test_refusals():
    q, kc, vc, cu, kn, vn, lens, table = _problem(torch.float32, D, H, HK, COUNTS, CACHED, 64, 0, 5)
    call = lambda s: alibi(q, kc.clone(), vc.clone(), cu, kn, vn, cache_seqlens=lens, alibi_slopes=s)
    with pytest.raises(TypeError, match="float32"):
        call(_slopes().double())
    with pytest.raises(TypeError, match="float32"):
        call([0.5] * H)
    for bad in (_slopes(H + 1), _slopes()[None].expand(len(COUNTS) + 1, H), torch.tensor(0.5), _slopes().reshape(H, 1)):
        with pytest.raises(ValueError, match="alibi_slopes must have shape"):
            call(bad)
    for value in (float("nan"), float("inf")):
        s = _slopes()
        s[2] = value
        with pytest.raises(ValueError, match="finite"):
            call(s)
    with pytest.raises(RuntimeError, match="forward-only"):
        alibi(q.clone().requires_grad_(), kc.clone(), vc.clone(), cu, kn, vn, cache_seqlens=lens, alibi_slopes=_slopes())
    # the existing refusal stays: a window takes no attn_bias on the CPU path
    from flash_cosine_sim_attention_amd import cpu
    with pytest.raises(ValueError, match="no mask and no attn_bias"):
        cpu.attention_forward_cpu(q[None, :, :, :].transpose(1, 2), q[None].transpose(1, 2), q[None].transpose(1, 2),
                                  attn_bias=torch.zeros(H, sum(COUNTS), sum(COUNTS)), window_size=(3, 0))
    # and the tree path takes no slopes
    with pytest.raises(ValueError, match="tree_mask"):
        cpu.attention_forward_kvcache_varlen_cpu(q, kc.clone(), vc.clone(), cu, kn, vn, CACHED, tree_mask=torch.zeros(sum(COUNTS), dtype=torch.int64),
                                                 alibi_slopes=_slopes())


def test_the_op_has_its_own_namespace_a_pinned_schema_and_no_autograd_kernel():
    _torch_ops.load()
    names = {n.split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith("fcsa_alibi::")}
    assert names == {"fcsa_alibi::kvcache_alibi_forward"}
    op = torch.ops.fcsa_alibi.kvcache_alibi_forward
    assert op.overloads() == ["default"]
    assert str(op.default._schema) == SCHEMA
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("fcsa_alibi::kvcache_alibi_forward", "Autograd")
    assert torch._C._dispatch_has_kernel_for_dispatch_key("fcsa_alibi::kvcache_alibi_forward", "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("fcsa_alibi::kvcache_alibi_forward", "CPU")


def _fake_args(mode_tensor=torch.empty):
    q = mode_tensor(7, 8, 128, dtype=torch.float16)
    kc = mode_tensor(2, 2, 64, 128, dtype=torch.float16)
    cu = mode_tensor(3, dtype=torch.int32)
    return (q, kc, kc.clone(), cu, mode_tensor(2, 8), None, None, None, None, None, None, 7, 64, 8.0, True, True, 1, 40, -1, 512, -1, False, False)


def test_fake_kernel_gives_the_shapes_and_passes_opcheck():
    from torch._subclasses.fake_tensor import FakeTensorMode
    _torch_ops.load()
    with FakeTensorMode():
        o, lse = torch.ops.fcsa_alibi.kvcache_alibi_forward(*_fake_args())
    assert o.shape == (7, 8, 128) and o.dtype == torch.float16 and lse.shape == (7, 8) and lse.dtype == torch.float32
    # opcheck of the registrations that need no device: the schema (mutated caches declared) and the fake kernel's consistency on meta tensors
    meta = _fake_args(lambda *s, **k: torch.empty(*s, device="meta", **k))
    torch.library.opcheck(torch.ops.fcsa_alibi.kvcache_alibi_forward, meta, test_utils=("test_schema", "test_faketensor"))


def test_c_entry_is_exported_declared_and_refuses_before_any_launch():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fcsa.h")).read()
    sym = "fcsa_forward_kvcache_alibi"
    assert sym in _lib.EXPORTS and hasattr(lib, sym)
    assert re.search(r"^int\s+" + sym + r"\(", header, flags=re.M)
    assert lib.fcsa_debug(None, 0) == 4 == _lib.ABI_VERSION      # additive: the ABI version stays
    assert [n for n, _ in _lib.Alibi._fields_] == ["slopes", "stride_b", "stride_h", "reserved"] and C.sizeof(_lib.Alibi) == 32
    fa, kv, seqs, st = _lib.ForwardArgs(), _lib.KvCache(), _lib.Varlen(), _lib.KvCacheStep()
    fa.p = _lib.problem(torch.bfloat16, (2, 8, 2, 4, 64, 64), True, False, True, 1, 8.0)
    kv.capacity = 64
    seqs.total_q = 5
    seqs.cu_seqlens_q = 4096
    fa.q = fa.o = _lib.Tensor(1 << 20, 0, 64, 8 * 64)                                  # (synthetic addresses: every call is refused before any launch)
    kv.k_cache = kv.v_cache = _lib.Tensor(1 << 24, 2 * 64 * 64, 64 * 64, 64)
    call = lambda al: lib.fcsa_forward_kvcache_alibi(C.byref(fa), C.byref(kv), C.byref(seqs), None, None, C.byref(st), al, None)
    assert call(None) == -1 and b"kvcache_alibi: null argument" in lib.fcsa_last_error()
    assert call(C.byref(_lib.Alibi(None, 0, 1, 0))) == -1 and b"slopes: null pointer" in lib.fcsa_last_error()
    assert call(C.byref(_lib.Alibi((1 << 22) + 2, 0, 1, 0))) == -1 and b"4-byte aligned" in lib.fcsa_last_error()
    assert call(C.byref(_lib.Alibi(1 << 22, 0, 1, 9))) == -1 and b"reserved" in lib.fcsa_last_error()
    assert lib.fcsa_forward_kvcache_alibi(None, None, None, None, None, None, None, None) == -1
    # with good slopes the step call's own checks follow: its flags are still flags
    bad = _lib.KvCacheStep(128, 2, -1, 0, 0)
    good = _lib.Alibi(1 << 22, 0, 1, 0)
    assert lib.fcsa_forward_kvcache_alibi(C.byref(fa), C.byref(kv), C.byref(seqs), None, None, C.byref(bad), C.byref(good), None) == -1
    assert b"are flags" in lib.fcsa_last_error()
    doc = " ".join(header.replace("\n *", " ").split())
    for text in ('"alibi_decode[_fp8]"', '"alibi_prefill[_fp8]"', "FCSA_ABI_VERSION stays 4", "per-row-shift regime", "|pos_i - j|"):
        assert text in doc, text


# ---- the CPU path against the float64 oracle ------------------------------------------------------------------------------------------------
def _band(n, L, left, right, causal):
    i = np.arange(n)[:, None] + (L - n)
    j = np.arange(L)[None]
    ok = np.ones((n, L), bool)
    if left >= 0:
        ok &= j >= i - left
    r = 0 if causal else right
    if r >= 0:
        ok &= j <= i + r
    return np.where(ok, 0.0, -np.inf)[None]


@pytest.mark.parametrize("per_sequence", [False, True])
@pytest.mark.parametrize("name,kw", [("causal", dict(causal=True)), ("noncausal", dict(causal=False)),
                                     ("window", dict(causal=False, window_size=(9, 2)))])
def test_cpu_path_against_the_float64_oracle(name, kw, per_sequence):
    from oracle import cosine_sim_oracle as O
    cap = 64
    q, kc, vc, cu, kn, vn, lens, _ = _problem(torch.float32, D, H, HK, COUNTS, CACHED, cap, 0, 7)
    slopes = _slopes()
    if per_sequence:
        slopes = (slopes[None] * (1 + torch.arange(len(COUNTS), dtype=torch.float32)[:, None])).contiguous()
    o, lse = alibi(q, kc, vc, cu, kn, vn, cache_seqlens=lens, return_lse=True, alibi_slopes=slopes, **kw)
    left, right = kw.get("window_size", (-1, -1))
    cq = cu.tolist()
    npf = lambda t: t.double().numpy()
    for b, n in enumerate(COUNTS):
        if n == 0:
            continue
        L = CACHED[b] + n
        qb = npf(q[cq[b]:cq[b + 1]].permute(1, 0, 2))[None]
        kb, vb = (np.repeat(npf(t[b, :, :L])[None], H // HK, axis=1) for t in (kc, vc))      # the call appended in place
        sl = npf(slopes if slopes.dim() == 1 else slopes[b])
        i = np.arange(n)[:, None] + (L - n)
        bias = _band(n, L, left, right, kw["causal"]) - sl[:, None, None] * np.abs(i - np.arange(L)[None])[None]
        ref = O.attention_forward_stats(qb, kb, vb, scale=8.0, groups=1, causal=kw["causal"], l2norm_qk=True, attn_bias=bias, eps=1e-300)[0]
        got = npf(o[cq[b]:cq[b + 1]].permute(1, 0, 2))
        # float32 arithmetic against float64: 2^-24 relative per operation over D = 64 products and L <= 64 keys, logits of magnitude <= 8 + bias
        assert np.abs(got - ref[0]).max() <= 2e-5, (name, b, np.abs(got - ref[0]).max())
        qn, kn64 = (x / np.linalg.norm(x, axis=-1, keepdims=True) for x in (qb, kb))
        s = 8.0 * np.einsum("bhid,bhjd->bhij", qn, kn64)[0] + bias
        ref_lse = np.log(np.exp(s - s.max(-1, keepdims=True)).sum(-1)) + s.max(-1)
        assert np.abs(npf(lse[cq[b]:cq[b + 1]]).T - ref_lse).max() <= 2e-5, (name, b)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
