"""flash_cosine_sim_attention_prefill_with_kvcache without a GPU: its signature is the ragged call's, CPU tensors give exactly what the ragged
CPU path gives (contiguous and paged caches, append, causal, return_lse), every refusal is raised on CPU tensors too and names the ragged
call, the op lives in a namespace of its own with a pinned schema and no Autograd kernel, and the C ABI exports and documents the entry
point."""
import inspect
import os

import pytest
import torch

import flash_cosine_sim_attention_amd as F
from flash_cosine_sim_attention_amd import _lib, _torch_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
prefill = F.flash_cosine_sim_attention_prefill_with_kvcache
ragged = F.flash_cosine_sim_attention_varlen_with_kvcache
RAGGED_NAME = "flash_cosine_sim_attention_varlen_with_kvcache"

SCHEMA = ("fcsa_prefill::kvcache_prefill_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor cu_seqlens_q, Tensor? k_new, "
          "Tensor? v_new, Tensor? cache_seqlens, Tensor? block_table, int max_seqlen_q, int max_seqlen_k, float scale, bool causal, "
          "bool l2norm_qk, int groups) -> (Tensor, Tensor)")


def test_signature_is_the_ragged_calls():
    assert inspect.signature(prefill) == inspect.signature(ragged)
    assert list(inspect.signature(prefill).parameters) == [
        "q", "k_cache", "v_cache", "cu_seqlens_q", "k_new", "v_new", "cache_seqlens", "block_table", "max_seqlen_q", "max_seqlen_k", "scale", "groups",
        "causal", "l2norm_qk", "k_scale", "v_scale", "return_lse", "window_size"]
    assert "flash_cosine_sim_attention_prefill_with_kvcache" in F.__all__
    doc = prefill.__doc__
    assert "NO key splits" in doc and RAGGED_NAME in doc      # says what it is for and points small steps to the ragged call


def _problem(dtype, D, H, Hk, counts, cached, capacity, page, seed):
    g = torch.Generator().manual_seed(seed)
    B, total = len(counts), sum(counts)
    cu = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32)
    q = torch.randn(total, H, D, generator=g).to(dtype)
    kn, vn = torch.randn(total, Hk, D, generator=g).to(dtype), torch.randn(total, Hk, D, generator=g).to(dtype)
    if page:
        per = capacity // page
        table = torch.randperm(B * per, generator=g).to(torch.int32).view(B, per)
        kc, vc = torch.randn(B * per, Hk, page, D, generator=g).to(dtype), torch.randn(B * per, Hk, page, D, generator=g).to(dtype)
    else:
        table = None
        kc, vc = torch.randn(B, Hk, capacity, D, generator=g).to(dtype), torch.randn(B, Hk, capacity, D, generator=g).to(dtype)
    return q, kc, vc, cu, kn, vn, torch.tensor(cached, dtype=torch.int32), table


@pytest.mark.parametrize("page", [0, 16])
@pytest.mark.parametrize("append", [True, False])
@pytest.mark.parametrize("causal", [False, True])
def test_cpu_tensors_take_the_ragged_cpu_path(page, append, causal):
    """same arguments through both functions: o, lse and the caches afterwards are equal bit for bit"""
    q, kc, vc, cu, kn, vn, lens, table = _problem(torch.bfloat16, 64, 6, 2, [1, 0, 5, 40], [0, 17, 30, 3], 64, page, 3)
    outs = []
    for fn in (prefill, ragged):
        k1, v1 = kc.clone(), vc.clone()
        with torch.no_grad():
            o, lse = fn(q, k1, v1, cu, kn if append else None, vn if append else None, cache_seqlens=lens, block_table=table, scale=6, groups=2,
                        causal=causal, return_lse=True)
            o2 = fn(q, k1.clone(), v1.clone(), cu, None, None, cache_seqlens=lens + (torch.tensor([1, 0, 5, 40], dtype=torch.int32) if append else 0),
                    block_table=table, scale=6, groups=2, causal=causal)
        outs.append((o, lse, k1, v1, o2))
    for a, b in zip(*outs):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32), b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32))
    o, lse = outs[0][0], outs[0][1]
    assert lse.dtype == torch.float32 and lse.shape == (q.shape[0], q.shape[1])
    if append:
        assert not torch.equal(outs[0][2], kc)      # the append landed in the cache it was given
    if causal and not append:      # sequence 3: 40 tokens against 3 cached positions -> rows without a visible key
        assert torch.isinf(lse[6:6 + 37]).all() and (lse[6:6 + 37] < 0).all() and (o[6:6 + 37] == 0).all()


def test_refusals_name_the_ragged_call():
    """float32; fp8 caches and scales; D in {16, 32, 96}; a window: refused before the device branch, so on CPU tensors too"""
    def args(dtype=torch.bfloat16, D=64, cache_dtype=None):
        q, kc, vc, cu, kn, vn, lens, table = _problem(torch.float32, D, 4, 2, [3, 2], [5, 0], 16, 0, 1)
        cd = cache_dtype or dtype
        return (q.to(dtype), kc.to(cd), vc.to(cd), cu, kn.to(dtype), vn.to(dtype)), dict(cache_seqlens=lens)
    with torch.no_grad():
        a, kw = args(torch.float32)
        with pytest.raises(TypeError, match=RAGGED_NAME):
            prefill(*a, **kw)
        a, kw = args(cache_dtype=torch.float8_e4m3fn)
        with pytest.raises(TypeError, match=RAGGED_NAME):
            prefill(*a, **kw)
        a, kw = args()
        for scales in (dict(k_scale=1.0), dict(v_scale=torch.ones(2)), dict(k_scale=1.0, v_scale=1.0)):
            with pytest.raises(TypeError, match=RAGGED_NAME):
                prefill(*a, **kw, **scales)
        for D in (16, 32, 96):
            a, kw = args(D=D)
            with pytest.raises(ValueError, match=f"got {D}.*{RAGGED_NAME}"):
                prefill(*a, **kw)
        a, kw = args()
        for w in ((4, -1), (-1, 0), (3, 3)):
            with pytest.raises(ValueError, match=RAGGED_NAME):
                prefill(*a, **kw, window_size=w)
        with pytest.raises(TypeError, match="q's dtype"):      # mixed 16-bit types
            prefill(a[0], a[1].to(torch.float16), a[2].to(torch.float16), *a[3:], **kw)
        # and what the ragged call refuses stays refused: host tables, return_lse, grad
        with pytest.raises(ValueError, match="outside"):
            prefill(*a, cache_seqlens=torch.tensor([15, 0], dtype=torch.int32))
        with pytest.raises(TypeError):
            prefill(*a, **kw, return_lse=1)
    a, kw = args()
    with pytest.raises(RuntimeError, match="forward-only"):
        prefill(a[0].requires_grad_(), *a[1:], **kw)


def test_the_op_has_its_own_namespace_a_pinned_schema_and_no_autograd_kernel():
    _torch_ops.load()
    names = {n for n in torch._C._dispatch_get_all_op_names() if n.startswith("fcsa_prefill::")}
    assert {n.split(".")[0] for n in names} == {"fcsa_prefill::kvcache_prefill_forward"}
    op = torch.ops.fcsa_prefill.kvcache_prefill_forward
    assert op.overloads() == ["default"]
    assert str(op.default._schema) == SCHEMA
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("fcsa_prefill::kvcache_prefill_forward", "Autograd")
    assert torch._C._dispatch_has_kernel_for_dispatch_key("fcsa_prefill::kvcache_prefill_forward", "CUDA")
    assert not any(n.startswith("fcsa::kvcache_prefill") for n in torch._C._dispatch_get_all_op_names())


def test_fake_kernel_gives_the_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    _torch_ops.load()
    with FakeTensorMode():
        q = torch.empty(7, 8, 128, dtype=torch.bfloat16)
        kc = torch.empty(2, 2, 64, 128, dtype=torch.bfloat16)
        cu = torch.empty(3, dtype=torch.int32)
        o, lse = torch.ops.fcsa_prefill.kvcache_prefill_forward(q, kc, kc.clone(), cu, None, None, None, None, 7, 64, 8.0, True, True, 1)
    assert o.shape == (7, 8, 128) and o.dtype == torch.bfloat16 and lse.shape == (7, 8) and lse.dtype == torch.float32


def test_c_abi_exports_and_documents_the_entry_point():
    assert "fcsa_forward_kvcache_prefill" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "fcsa_forward_kvcache_prefill")
    assert lib.fcsa_debug(None, 0) == 4      # additive: the ABI version stays
    assert lib.fcsa_forward_kvcache_prefill(None, None, None, None) == -1 and b"kvcache_prefill: null argument" in lib.fcsa_last_error()
    header = open(os.path.join(ROOT, "include", "fcsa.h")).read()
    assert "int    fcsa_forward_kvcache_prefill(const fcsa_forward_args* args, const fcsa_kvcache* cache, const fcsa_varlen* seqs," in header
    assert '"kv_append_ragged"' in header and '"prefill"' in header
    for text in (header, open(os.path.join(ROOT, "README.md")).read(), open(os.path.join(ROOT, "DESIGN.md")).read()):
        assert "a prefill kernel reading a paged cache is not built" not in " ".join(text.split())
