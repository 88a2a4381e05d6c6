"""Tree attention against MXFP4 caches without a GPU: the public names and signature, the ops of the fcsa_mx_tree namespace and their fake kernels,
the C symbols and their refusals (synthetic addresses: no launch), the wrapper's refusals, and the CPU paths against the oracle and torch indexing."""
import ctypes as C
import inspect

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import flash_cosine_sim_attention_amd as F
import tree_cases as TC
from flash_cosine_sim_attention_amd import _lib, _torch_ops

FN = F.flash_cosine_sim_attention_mxfp4_tree_with_kvcache
COUNTS, CACHED, CAP, H, HK = [1, 0, 5, 30, 65], [0, 17, 21, 9, 40], 112, 6, 2
SYMBOLS = ("fcsa_forward_kvcache_mx_tree", "fcsa_forward_kvcache_mx_tree_workspace_bytes", "fcsa_kvcache_mx_compact")


def _make(D, dtype=torch.bfloat16, seed=0, paged=False):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    total, B = sum(COUNTS), len(COUNTS)
    (kc, ks), (vc, vs) = F.mxfp4_quantize(rnd(B, HK, CAP, D)), F.mxfp4_quantize(rnd(B, HK, CAP, D))
    table = None
    if paged:      # pages of 16 in a shuffled pool
        mb = CAP // 16
        table = torch.randperm(B * mb, generator=g).reshape(B, mb).to(torch.int32)
        pool = lambda t: t.unflatten(2, (mb, 16)).permute(0, 2, 1, 3, 4).flatten(0, 1)[torch.argsort(table.flatten())].contiguous()
        kc, vc, ks, vs = (pool(t) for t in (kc, vc, ks, vs))
    return rnd(total, H, D).to(dtype), [kc, vc, ks, vs], rnd(total, HK, D).to(dtype), rnd(total, HK, D).to(dtype), table


def test_public_names_and_signature():
    assert {"flash_cosine_sim_attention_mxfp4_tree_with_kvcache", "mxfp4_kvcache_keep_accepted"} <= set(F.__all__)
    base = list(inspect.signature(F.flash_cosine_sim_attention_mxfp4_with_kvcache).parameters.values())
    tree = list(inspect.signature(FN).parameters.values())
    assert len(base) == 18 and tree[:18] == base and tree[18].name == "tree_mask" and tree[18].default is None and len(tree) == 19
    assert list(inspect.signature(F.mxfp4_kvcache_keep_accepted).parameters) == ["k_cache", "v_cache", "k_block_scale", "v_block_scale", "cache_seqlens",
                                                                              "accepted", "num_accepted", "block_table"]
    q, mx, kn, vn, _ = _make(64)      # tree_mask=None IS the MXFP4 call
    sl, cu = torch.tensor(CACHED, dtype=torch.int32), TC.cu_of(COUNTS)
    a, b = [t.clone() for t in mx], [t.clone() for t in mx]
    got = FN(q, *a, cu, kn, vn, sl, causal=True, return_lse=True)
    want = F.flash_cosine_sim_attention_mxfp4_with_kvcache(q, *b, cu, kn, vn, sl, causal=True, return_lse=True)
    assert all(torch.equal(x, y) for x, y in zip([*got, *a], [*want, *b]))


def test_ops_schemas_fake_kernels_and_symbols():
    assert set(SYMBOLS) <= set(_lib.EXPORTS) and all(hasattr(_lib.load(), s) for s in SYMBOLS) and _lib.load().fcsa_debug(None, 0) == _lib.ABI_VERSION == 4
    _torch_ops.load()
    assert sorted(n.split("::")[1] for n in torch._C._dispatch_get_all_op_names() if n.startswith("fcsa_mx_tree::")) == ["kvcache_mxfp4_compact",
                                                                                                                        "kvcache_mxfp4_tree_forward"]
    assert str(torch.ops.fcsa_mx_tree.kvcache_mxfp4_tree_forward.default._schema) == (
        "fcsa_mx_tree::kvcache_mxfp4_tree_forward(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor(c!) k_block_scale, Tensor(d!) v_block_scale, "
        "Tensor cu_seqlens_q, Tensor tree_mask, Tensor? k_new, Tensor? v_new, Tensor? cache_seqlens, Tensor? block_table, int max_seqlen_q, "
        "int max_seqlen_k, float scale, bool l2norm_qk, int groups, bool return_lse) -> (Tensor, Tensor)")
    assert str(torch.ops.fcsa_mx_tree.kvcache_mxfp4_compact.default._schema) == (
        "fcsa_mx_tree::kvcache_mxfp4_compact(Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor(c!) k_block_scale, Tensor(d!) v_block_scale, "
        "Tensor cache_seqlens, Tensor accepted, Tensor num_accepted, Tensor? block_table) -> ()")
    for name in ("fcsa_mx_tree::kvcache_mxfp4_tree_forward", "fcsa_mx_tree::kvcache_mxfp4_compact"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(name, "CUDA")
        assert not any(torch._C._dispatch_has_kernel_for_dispatch_key(name, k) for k in ("Autograd", "CPU"))
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32)
    for want_lse in (False, True):      # the fake kernels: o like q, the lse empty unless asked for; the compaction returns nothing
        with FakeTensorMode():
            q, kc, ks = torch.empty(8, 4, 64, dtype=torch.bfloat16), torch.empty(2, 2, 32, 32, dtype=torch.uint8), torch.empty(2, 2, 32, 2, dtype=torch.uint8)
            o, lse = torch.ops.fcsa_mx_tree.kvcache_mxfp4_tree_forward(q, kc, kc, ks, ks, i32(3), torch.empty(8, dtype=torch.int64), None, None, None, None,
                                                                       8, 32, 8.0, True, 1, want_lse)
            assert o.shape == q.shape and o.dtype == q.dtype and lse.shape == ((8, 4) if want_lse else (0,)) and lse.dtype == torch.float32
            assert torch.ops.fcsa_mx_tree.kvcache_mxfp4_compact(kc, kc, ks, ks, i32(2), i32(2, 4), i32(2), None) is None


def _c_call(D=128, dtype=torch.bfloat16, causal=0, window=None, mask=0x2000, reserved=0, rows=True):
    """fcsa_forward_kvcache_mx_tree on synthetic (never dereferenced) addresses: every refusal happens before any launch"""
    lib = _lib.load()
    a = _lib.ForwardArgs()
    a.p = _lib.problem(dtype, (2, 8, 2, 8, 64, D), causal=bool(causal))
    a.q = a.o = _lib.Tensor(0x10000, 0, D, 8 * D)
    kv, mx, seqs = _lib.KvCache(), _lib.KvCacheMx(), _lib.Varlen()
    kv.k_cache = kv.v_cache = _lib.Tensor(0x20000, 2 * 64 * D // 2, 64 * D // 2, D // 2)
    kv.capacity = 64
    mx.format = _lib.FCSA_CACHE_MXFP4
    mx.k_block_scale = mx.v_block_scale = _lib.Tensor(0x30000, 2 * 64 * (D // 32), 64 * (D // 32), D // 32)
    seqs.cu_seqlens_q, seqs.total_q = 0x40000, 16 if rows else 0
    tree = _lib.TreeMask(mask, reserved)
    win = None if window is None else C.byref(_lib.Window(*window))
    rc = lib.fcsa_forward_kvcache_mx_tree(C.byref(a), C.byref(kv), C.byref(mx), C.byref(seqs), win, C.byref(tree), None)
    ws = lib.fcsa_forward_kvcache_mx_tree_workspace_bytes(C.byref(a.p), C.byref(kv), C.byref(mx), C.byref(seqs))
    return rc, ws, lib.fcsa_last_error().decode()


def test_c_entry_refusals():
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4      # FCSA_ERR_INVALID_ARG, FCSA_ERR_UNSUPPORTED, FCSA_ERR_WORKSPACE
    lib = _lib.load()
    assert lib.fcsa_forward_kvcache_mx_tree(None, None, None, None, None, None, None) == INVALID
    assert lib.fcsa_kvcache_mx_compact(None, None, 1, 1, 128, None, 4, 4, None, None) == INVALID
    assert all(_c_call(D=D)[:2] == (UNSUPPORTED, 0) and "64 or 128" in _c_call(D=D)[2] for D in (32, 96))
    rc, ws, msg = _c_call(dtype=torch.float32)
    assert rc == UNSUPPORTED and ws == 0 and "f16 or bf16" in msg and _c_call(causal=1)[0] == INVALID and "causal" in _c_call(causal=1)[2]
    assert _c_call(window=(4, -1))[0] == INVALID and _c_call(window=(-1, 0))[0] == INVALID and "window" in _c_call(window=(4, -1))[2]
    assert _c_call(mask=0)[0] == INVALID and "mask: null" in _c_call(mask=0)[2]
    assert _c_call(mask=0x2004)[0] == INVALID and _c_call(reserved=1)[0] == INVALID
    rc, ws, msg = _c_call()      # past every refusal the call asks for its workspace (none was given); without rows it launches nothing
    assert rc == WORKSPACE and ws > 0 and "kvcache_mx_tree" in msg
    assert _c_call(rows=False, window=(-1, -1))[:2] == (0, 0)


def test_wrapper_refusals():
    q, mx, kn, vn, _ = _make(64)
    sl, cu, words = torch.tensor(CACHED, dtype=torch.int32), TC.cu_of(COUNTS), TC.as_int64(TC.words_of("tree", COUNTS))
    small, odd = _make(32), _make(96)
    acc, n = torch.tensor([[0, 1]] * 5, dtype=torch.int32), torch.tensor([2] * 5, dtype=torch.int32)
    keep, tree16 = F.mxfp4_kvcache_keep_accepted, F.flash_cosine_sim_attention_tree_with_kvcache
    for exc, match, call in [
            (ValueError, "packed queries", lambda: FN(q[None].transpose(1, 2), *mx, None, cache_seqlens=sl, tree_mask=words)),
            (ValueError, "causal=True cannot", lambda: FN(q, *mx, cu, kn, vn, sl, causal=True, tree_mask=words)),
            (ValueError, "no sliding window", lambda: FN(q, *mx, cu, kn, vn, sl, window_size=(8, 0), tree_mask=words)),
            (TypeError, "int64", lambda: FN(q, *mx, cu, kn, vn, sl, tree_mask=words.int())),
            (ValueError, "one word per packed query row", lambda: FN(q, *mx, cu, kn, vn, sl, tree_mask=words[:-1])),
            (TypeError, "float16 or bfloat16 q at dim_head 64 or 128", lambda: FN(q.float(), *mx, cu, kn.float(), vn.float(), sl, tree_mask=words)),
            (ValueError, "dim_head 64 or 128", lambda: FN(small[0], *small[1], cu, small[2], small[3], sl, tree_mask=words)),
            (ValueError, "dim_head 64 or 128", lambda: FN(odd[0], *odd[1], cu, odd[2], odd[3], sl, tree_mask=words)),
            (TypeError, "mxfp4", lambda: tree16(q, mx[0], mx[1], cu, cache_seqlens=sl, tree_mask=words)),      # uint8 caches: an MXFP4 function is named
            (TypeError, "torch.uint8", lambda: keep(mx[0].float(), mx[1].float(), mx[2], mx[3], sl, acc, n)),
            (ValueError, "k_block_scale must be", lambda: keep(mx[0], mx[1], mx[2][..., :1], mx[3], sl, acc, n)),
            (ValueError, "strictly increasing", lambda: keep(*mx, sl, torch.tensor([[1, 1]] * 5, dtype=torch.int32), n))]:
        with pytest.raises(exc, match=match):
            call()


@pytest.mark.parametrize("dtype,D,paged,kw", [("bf16", 64, False, {}), ("f16", 128, True, dict(groups=2)), ("bf16", 128, False, dict(l2norm_qk=False, scale=0.1))])
def test_cpu_path_against_the_oracle(dtype, D, paged, kw):
    """quantise and append, dequantise, cpu.py's tree path: the bytes of mxfp4_quantize at the step's slots, and o against the float64
    oracle with the tree visibility on the dequantised caches, under the type's forward bars (the GPU tests' reference and check)"""
    import cases
    import test_gpu_kvcache as TK
    import test_gpu_kvcache_tree as TT
    q, mx, kn, vn, table = _make(D, TK.DT[dtype], seed=D, paged=paged)
    words = [0] + TC.words_of("tree", COUNTS, D)[1:]      # the one token of the empty cache sees nothing
    before = [t.clone() for t in mx]
    o, lse = FN(q, *mx, TC.cu_of(COUNTS), kn, vn, torch.tensor(CACHED, dtype=torch.int32), table, return_lse=True, tree_mask=TC.as_int64(words), **kw)
    assert (o[0] == 0).all() and torch.isneginf(lse[0]).all() and not torch.isnan(lse).any()
    cu, lens = TC.cu_of(COUNTS).tolist(), [s + n for s, n in zip(CACHED, COUNTS)]
    rows = lambda t: TK._seqs(t, t, lens, table)[0]      # every sequence's positions [0, L_b) of a cache tensor
    (kc, ks), (vc, vs) = F.mxfp4_quantize(kn), F.mxfp4_quantize(vn)
    for got, old, fresh in zip(mx, before, (kc, vc, ks, vs)):
        for b, s in enumerate(CACHED):
            assert torch.equal(rows(got)[b][:, :s], rows(old)[b][:, :s]) and torch.equal(rows(got)[b][:, s:], fresh[cu[b]:cu[b + 1]].transpose(0, 1))
    kseq, vseq = TK._seqs(F.mxfp4_dequantize(mx[0], mx[2], q.dtype), F.mxfp4_dequantize(mx[1], mx[3], q.dtype), lens, table)
    cond = cases.logit_cond(dtype, kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True))
    TK._check(dtype, o, TT._reference(q, COUNTS, kseq, vseq, words, kw), f"mxfp4_tree_cpu/{dtype}/{D}", cond)


@pytest.mark.parametrize("paged", [False, True])
def test_keep_accepted_cpu_path(paged):
    """all four tensors byte-equal to the same moves done with torch indexing on a copy: identity, shift by one, scattered, empty"""
    _, mx, _, _, table = _make(64, seed=3, paged=paged)
    seq, count = [3, 20, 31, 64, 0], [4, 5, 5, 0, 1]
    accepted = [[0, 1, 2, 3, 0], [1, 2, 3, 4, 5], [0, 5, 9, 30, 63], [7, 8, 9, 10, 11], [2, 0, 0, 0, 0]]
    dense = (lambda t: t) if table is None else (lambda t: torch.stack([torch.cat([t[int(i)] for i in table[b]], dim=1) for b in range(len(seq))]))
    want = [dense(t).clone() for t in mx]
    for b, (s, n) in enumerate(zip(seq, count)):
        for t in want:
            t[b, :, s:s + n] = t[b, :, [s + a for a in accepted[b][:n]]].clone()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    assert F.mxfp4_kvcache_keep_accepted(*mx, i32(seq), i32(accepted), i32(count), table) is None
    assert all(torch.equal(dense(got), ref) for got, ref in zip(mx, want))
