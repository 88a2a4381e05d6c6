"""The 64-row verify call of float16 / bfloat16 / fp8 caches without a GPU: the public name and signature, the op of the fcsa_verify namespace
and its fake kernel, the C symbols and their refusals (synthetic addresses: no launch), the wrapper's refusals, and the CPU path."""
import ctypes as C
import inspect

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import flash_cosine_sim_attention_amd as F
import tree_cases as TC
from flash_cosine_sim_attention_amd import _lib, _torch_ops

FN = F.flash_cosine_sim_attention_verify_with_kvcache
TREE = F.flash_cosine_sim_attention_tree_with_kvcache
COUNTS, CACHED, CAP, H, HK = [1, 0, 5, 30, 65], [0, 17, 21, 9, 40], 112, 6, 2
SYMBOLS = ("fcsa_forward_kvcache_verify", "fcsa_forward_kvcache_verify_workspace_bytes")


def _make(D, dtype=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dtype)
    total = sum(COUNTS)
    return rnd(total, H, D), rnd(len(COUNTS), HK, CAP, D), rnd(len(COUNTS), HK, CAP, D), rnd(total, HK, D), rnd(total, HK, D)


def test_public_name_and_signature():
    assert "flash_cosine_sim_attention_verify_with_kvcache" in F.__all__
    assert inspect.signature(FN) == inspect.signature(TREE) and len(inspect.signature(FN).parameters) == 19
    assert list(inspect.signature(FN).parameters)[-1] == "tree_mask" and inspect.signature(FN).parameters["tree_mask"].default is None


def test_op_schema_fake_kernel_and_symbols():
    assert set(SYMBOLS) <= set(_lib.EXPORTS) and all(hasattr(_lib.load(), s) for s in SYMBOLS) and _lib.load().fcsa_debug(None, 0) == _lib.ABI_VERSION == 4
    _torch_ops.load()
    name = "fcsa_verify::kvcache_verify_forward"
    assert [n for n in torch._C._dispatch_get_all_op_names() if n.startswith("fcsa_verify::")] == [name]
    assert str(torch.ops.fcsa_verify.kvcache_verify_forward.default._schema) == (
        "fcsa_verify::kvcache_verify_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor cu_seqlens_q, Tensor? tree_mask, Tensor? k_new, "
        "Tensor? v_new, Tensor? cache_seqlens, Tensor? block_table, Tensor? k_scale, Tensor? v_scale, int max_seqlen_q, int max_seqlen_k, "
        "float scale, bool causal, bool l2norm_qk, int groups, bool return_lse) -> (Tensor, Tensor)")
    assert torch._C._dispatch_has_kernel_for_dispatch_key(name, "CUDA")
    assert not any(torch._C._dispatch_has_kernel_for_dispatch_key(name, k) for k in ("Autograd", "CPU"))
    for want_lse in (False, True):      # the fake kernel: o like q, the lse empty unless asked for
        with FakeTensorMode():
            q, kc = torch.empty(8, 4, 64, dtype=torch.bfloat16), torch.empty(2, 2, 32, 64, dtype=torch.bfloat16)
            o, lse = torch.ops.fcsa_verify.kvcache_verify_forward(q, kc, kc, torch.empty(3, dtype=torch.int32), None, None, None, None, None, None, None,
                                                                  8, 32, 8.0, True, True, 1, want_lse)
            assert o.shape == q.shape and o.dtype == q.dtype and lse.shape == ((8, 4) if want_lse else (0,)) and lse.dtype == torch.float32


def _c_call(D=128, dtype=torch.bfloat16, causal=0, mask=0x2000, reserved=0, rows=True, tree=True):
    """fcsa_forward_kvcache_verify on synthetic (never dereferenced) addresses: every refusal happens before any launch"""
    lib = _lib.load()
    a = _lib.ForwardArgs()
    a.p = _lib.problem(dtype, (2, 8, 2, 8, 64, D), causal=bool(causal))
    a.q = a.o = _lib.Tensor(0x10000, 0, D, 8 * D)
    kv, seqs = _lib.KvCache(), _lib.Varlen()
    kv.k_cache = kv.v_cache = _lib.Tensor(0x20000, 2 * 64 * D, 64 * D, D)
    kv.capacity = 64
    seqs.cu_seqlens_q, seqs.total_q = 0x40000, 16 if rows else 0
    tm = C.byref(_lib.TreeMask(mask, reserved)) if tree else None
    rc = lib.fcsa_forward_kvcache_verify(C.byref(a), C.byref(kv), C.byref(seqs), None, tm, None)
    ws = lib.fcsa_forward_kvcache_verify_workspace_bytes(C.byref(a.p), C.byref(kv), C.byref(seqs), None)
    return rc, ws, lib.fcsa_last_error().decode()


def test_c_entry_refusals():
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4      # FCSA_ERR_INVALID_ARG, FCSA_ERR_UNSUPPORTED, FCSA_ERR_WORKSPACE
    lib = _lib.load()
    assert lib.fcsa_forward_kvcache_verify(None, None, None, None, None, None) == INVALID
    assert lib.fcsa_forward_kvcache_verify_workspace_bytes(None, None, None, None) == 0
    rc, ws, msg = _c_call(D=96)
    assert (rc, ws) == (UNSUPPORTED, 0) and "64 or 128" in msg and "fcsa_forward_kvcache_tree" in msg
    rc, ws, msg = _c_call(dtype=torch.float32)
    assert (rc, ws) == (UNSUPPORTED, 0) and "f16 or bf16" in msg and "fcsa_forward_kvcache_tree" in msg
    assert _c_call(causal=1)[0] == INVALID and "causal" in _c_call(causal=1)[2]
    assert _c_call(mask=0)[0] == INVALID and "mask: null" in _c_call(mask=0)[2]
    assert _c_call(mask=0x2004)[0] == INVALID and _c_call(reserved=1)[0] == INVALID
    for kw in (dict(), dict(tree=False), dict(tree=False, causal=1)):      # past every refusal the call asks for its workspace (none was given)
        rc, ws, msg = _c_call(**kw)
        assert rc == WORKSPACE and ws > 0 and "kvcache_verify" in msg
    assert _c_call(rows=False)[:2] == (0, 0)      # without rows it launches nothing


def test_wrapper_refusals():
    q, kc, vc, kn, vn = _make(64)
    sl, cu, words = torch.tensor(CACHED, dtype=torch.int32), TC.cu_of(COUNTS), TC.as_int64(TC.words_of("tree", COUNTS))
    small, odd = _make(32), _make(96)
    codes = torch.zeros(len(COUNTS), HK, CAP, 32, dtype=torch.uint8)
    for exc, match, call in [
            (ValueError, "causal=True cannot", lambda: FN(q, kc, vc, cu, kn, vn, sl, causal=True, tree_mask=words)),
            (ValueError, "no sliding window", lambda: FN(q, kc, vc, cu, kn, vn, sl, window_size=(8, 0))),
            (ValueError, "no sliding window", lambda: FN(q, kc, vc, cu, kn, vn, sl, causal=True, window_size=(-1, 0))),
            (TypeError, "tree_with_kvcache takes float32", lambda: FN(q.float(), kc.float(), vc.float(), cu, kn.float(), vn.float(), sl, tree_mask=words)),
            (ValueError, "tree_with_kvcache takes the others", lambda: FN(small[0], small[1], small[2], cu, small[3], small[4], sl)),
            (ValueError, "tree_with_kvcache takes the others", lambda: FN(odd[0], odd[1], odd[2], cu, odd[3], odd[4], sl, tree_mask=words)),
            (TypeError, "flash_cosine_sim_attention_mxfp4_tree_with_kvcache", lambda: FN(q, codes, codes, cu, cache_seqlens=sl, tree_mask=words)),
            (ValueError, "packed queries", lambda: FN(q[None].transpose(1, 2), kc, vc, cu, cache_seqlens=sl)),
            (TypeError, "int64", lambda: FN(q, kc, vc, cu, kn, vn, sl, tree_mask=words.int())),
            (ValueError, "one word per packed query row", lambda: FN(q, kc, vc, cu, kn, vn, sl, tree_mask=words[:-1]))]:
        with pytest.raises(exc, match=match):
            call()


@pytest.mark.parametrize("dtype,D,how", [(torch.bfloat16, 64, "tree"), (torch.float16, 128, "bits"), (torch.bfloat16, 128, "causal"), (torch.float16, 64, "full")])
def test_cpu_tensors_take_the_tree_calls_cpu_path(dtype, D, how):
    """o, lse and the caches after the append equal the tree call's on CPU tensors: with a mask, and with tree_mask=None (there the tree call
    is the ragged call)"""
    q, kc, vc, kn, vn = _make(D, dtype, seed=D)
    sl, cu = torch.tensor(CACHED, dtype=torch.int32), TC.cu_of(COUNTS)
    kw = dict(causal=how == "causal") if how in ("causal", "full") else dict(tree_mask=TC.as_int64(TC.words_of(how, COUNTS, D)))
    a, b = [kc.clone(), vc.clone()], [kc.clone(), vc.clone()]
    got, want = FN(q, *a, cu, kn, vn, sl, return_lse=True, **kw), TREE(q, *b, cu, kn, vn, sl, return_lse=True, **kw)
    assert all(torch.equal(x, y) for x, y in zip([*got, *a], [*want, *b])) and not torch.isnan(got[1]).any()
