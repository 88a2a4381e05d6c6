"""Tree attention for speculative decoding on the GPU: flash_cosine_sim_attention_tree_with_kvcache (tree_mask; decode_tree[_fp8]_kernel,
fcsa_forward_kvcache_tree) and kvcache_keep_accepted (kv_compact_kernel, fcsa_kvcache_compact).

1. Identities, bit for bit: the chain mask is the ragged call with causal=True, all bits set the ragged call with causal=False -- o, lse and
   the cache bytes after the append.  The tree call is planned as the non-causal ragged call and differs from it in the per-logit
   visibility test alone, so this holds at one key split and at many.
2. Random trees and random bit sets against the float64 oracle with the mask as a 0 / -inf bias, under the project's forward bars.
3. The visibility probe (visibility_probe.py's cone inputs): a single hidden or leaked bit fails.
4. Graph capture, 5. buffer bounds through the C ABI, 6. the compaction of the accepted path, alone and inside a whole speculative step."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_kvcache as TK
import test_gpu_kvcache_fp8 as T8
import test_gpu_kvcache_ragged as TR
import tree_cases as TC
import visibility_probe as VP
from test_gpu_buffer_bounds import Arena

pytestmark = pytest.mark.gpu

DT = TK.DT
E4M3 = torch.float8_e4m3fn
_cu, _i32, _bits = TR._cu, TR._i32, TR._bits


def _api():
    """the tree call: the ragged call's arguments and tree_mask (without a mask it IS the ragged call)"""
    import flash_cosine_sim_attention_amd as F
    return F.flash_cosine_sim_attention_tree_with_kvcache


def _keep():
    import flash_cosine_sim_attention_amd as F
    return F.kvcache_keep_accepted


def _mask(kind, counts, seed=0):
    return TC.as_int64(TC.words_of(kind, counts, seed), "cuda")


def _raw(t):
    """a cache's bytes (fp8 caches have no comparison of their own)"""
    return t.view(torch.uint8) if t.dtype == E4M3 else _bits(t)


# ---- 1. identities, bit for bit -------------------------------------------------------------------------------------------------------------

def _identity(dtype, D, H, Hk, counts, cached, cap, layout, kw, seed, max_k=None):
    """chain == causal=True and all ones == causal=False on independent copies of the same caches: o, lse, the cache bytes"""
    q, kc, vc, kn, vn = TR._inputs(dtype, H, Hk, D, counts, cap, seed)
    quant = {}
    if layout.startswith("fp8"):
        (kc, ks), (vc, vs) = T8._quantise(kc), T8._quantise(vc)
        kc, vc = kc.view(torch.uint8), vc.view(torch.uint8)
        quant = dict(k_scale=ks, v_scale=vs)
    table = None
    if layout.endswith("paged"):
        kc, vc, table = TR._paged(kc, vc, 16, seed)
        table = table.cuda()
    typed = (lambda t: t.view(E4M3)) if quant else (lambda t: t)
    bounds = {} if max_k is None else dict(max_seqlen_k=max_k)

    def run(**how):
        k, v = kc.clone(), vc.clone()
        with torch.no_grad():
            fn = _api() if "tree_mask" in how else TR._api()          # (the reference side: the existing ragged call itself)
            o, lse = fn(q, typed(k), typed(v), _cu(counts), kn, vn, _i32(cached), block_table=table, return_lse=True, **bounds, **quant, **kw, **how)
        return o, lse, k, v

    for kind, causal in (("chain", True), ("full", False)):
        got, want = run(tree_mask=_mask(kind, counts)), run(causal=causal)
        torch.cuda.synchronize()
        for name, a, b in zip(("o", "lse", "k_cache", "v_cache"), got, want):
            assert torch.equal(_bits(a), _bits(b)), f"{kind}: {name}: {int((_bits(a) != _bits(b)).sum())} elements differ"
        assert not torch.isnan(got[1]).any()


REGIME_KW = (dict(), dict(scale=16.0, groups=2))          # scale 8; scale 16 with groups 2 (16-bit: the per-row-shift regime)
IDENTITIES = [(f"{dt}_d{d}_hk{hk}_{layout}", dt, d, hk, layout)
              for dt in ("bf16", "f16", "f32") for d in (16, 64, 96, 128) for hk in (8, 2, 1)
              for layout in (("contiguous", "paged") if dt == "f32" else ("contiguous", "paged", "fp8" if hk != 2 else "fp8_paged"))]


@pytest.mark.parametrize("name,dtype,D,Hk,layout", IDENTITIES, ids=[c[0] for c in IDENTITIES])
def test_chain_is_causal_and_all_ones_is_plain_at_one_split(name, dtype, D, Hk, layout):
    """one key split on both sides: max_seqlen_k = the capacity 240 < 2 * decode_min_split_keys(D), as test_gpu_kvcache_ragged.py arranges it"""
    for kw in REGIME_KW:
        _identity(dtype, D, 8, Hk, TC.N_B, TC.BIT_CACHED, TC.BIT_CAP, layout, kw, seed=sum(map(ord, name)), max_k=TC.BIT_CAP)


# a 20 000-key cache: many key splits.  The step's tokens straddle a 32-key block in every sequence (positions 19967 | 19968, 7663 .. 7699
# over 7680, 8987 .. 8995 over 8992), and at 16 splits the second sequence's L = 7700 puts its last split at [7680, 7700): inside the step
LONG_N, LONG_CACHED, LONG_CAP = [2, 37, 9], [19967, 7663, 8987], 20000
LONG = [("bf16_d128_hk2", "bf16", 128, 2, "contiguous"), ("f16_d64_hk2_fp8", "f16", 64, 2, "fp8"), ("f32_d32_hk1", "f32", 32, 1, "contiguous"),
        ("bf16_d16_hk2_paged", "bf16", 16, 2, "paged")]


@pytest.mark.parametrize("name,dtype,D,Hk,layout", LONG, ids=[c[0] for c in LONG])
def test_chain_is_causal_and_all_ones_is_plain_at_many_splits(name, dtype, D, Hk, layout):
    """the plan of both sides is the same by construction (the tree call is planned as the non-causal ragged call, whose plan does not look
    at causal), so the results are still bit-equal"""
    for kw in REGIME_KW:
        _identity(dtype, D, 8, Hk, LONG_N, LONG_CACHED, LONG_CAP, layout, kw, seed=len(name))


# ---- 2. random trees and random bit sets against the float64 oracle -------------------------------------------------------------------------

def _reference(q, counts, kseq, vseq, words, kw, operand_dtype=None):
    """the float64 oracle per sequence with the mask as a 0 / -inf attn_bias (the route test_gpu_kvcache_ragged._reference takes for
    windows); rows without a visible key are 0"""
    import cases
    from oracle import cosine_sim_oracle as O
    cu = _cu(counts, "cpu").tolist()
    out = np.zeros(q.shape)
    dtype = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}[q.dtype]
    scale, groups, l2 = kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True)
    dyn = cases.dynamic_shift_regime(dtype, scale, groups, l2, False)
    H = q.shape[1]
    for b, (n, own) in enumerate(zip(counts, TC.split_words(words, counts))):
        L = kseq[b].shape[1]
        if n == 0 or L == 0:
            continue
        vis = TC.visibility(own, n, L)
        dead = ~vis.any(1)
        vis[dead] = True                                   # (a row of -inf alone has no softmax: computed on all keys, then zeroed)
        G = H // kseq[b].shape[0]
        kr, vr = (np.repeat(TK._np(x)[None], G, axis=1) for x in (kseq[b], vseq[b]))
        o = O.attention_forward_stats(TK._np(TR._rows(q, cu, b)), kr, vr, scale=scale, groups=groups, causal=False, l2norm_qk=l2,
                                      attn_bias=np.repeat(TC.bias_of(vis), H, axis=0), eps=1e-300 if dyn else 1e-10, operand_dtype=operand_dtype)[0]
        o[:, :, dead] = 0.0
        out[cu[b]:cu[b + 1]] = o[0].transpose(1, 0, 2)
    return out


ORACLE_N = TC.N_B[:-1] + [70]                            # ... and a sequence of 70 tokens, which is causal
ORACLE = [("bf16_d128_hk2", "bf16", 128, 2, dict()), ("f16_d64_hk8", "f16", 64, 8, dict()), ("f32_d32_hk1", "f32", 32, 1, dict()),
          ("f32_d96_groups4_lds_form", "f32", 96, 2, dict(groups=4, scale=4.0)), ("f16_d64_per_row_regime", "f16", 64, 2, dict(scale=16.0, groups=2)),
          ("bf16_d16_hk1", "bf16", 16, 1, dict())]


@pytest.mark.parametrize("kind", ["tree", "bits"])
@pytest.mark.parametrize("name,dtype,D,Hk,kw", ORACLE, ids=[c[0] for c in ORACLE])
def test_random_masks_against_the_float64_oracle(name, dtype, D, Hk, kw, kind):
    """the bars of test_gpu_kvcache_ragged._verify: the raw pass scaled by cases.logit_cond and, 16-bit with l2norm, the operand-faithful pass"""
    import cases
    H, seed = 8, sum(map(ord, name))
    q, kc, vc, kn, vn = TR._inputs(dtype, H, Hk, D, ORACLE_N, TC.CAPACITY, seed)
    words = TC.words_of(kind, ORACLE_N, seed)
    words[0] = 0                                           # an empty cache and no bit set
    paged = seed % 2 == 1
    table = None
    if paged:
        kc, vc, table = TR._paged(kc, vc, 16, seed)
    with torch.no_grad():
        o, lse = _api()(q, kc, vc, _cu(ORACLE_N), kn, vn, _i32(TC.CACHED), block_table=None if table is None else table.cuda(), return_lse=True,
                        tree_mask=TC.as_int64(words, "cuda"), **kw)
    torch.cuda.synchronize()
    lens = [s + n for s, n in zip(TC.CACHED, ORACLE_N)]
    ks, vs = TK._seqs(kc, vc, lens, table)
    label = f"tree/{name}/{kind}"
    cond = cases.logit_cond(dtype, kw.get("scale", 8.0), kw.get("groups", 1), True)
    TK._check(dtype, o, _reference(q, ORACLE_N, ks, vs, words, kw), label + "/raw", cond)
    if dtype != "f32":
        TK._check(dtype, o, _reference(q, ORACLE_N, ks, vs, words, kw, operand_dtype=dtype), label + "/operands")
    # rows without a visible key: o == 0 and lse == -inf, and nowhere else
    dead = np.concatenate([~TC.visibility(own, n, L).any(1) for own, n, L in zip(TC.split_words(words, ORACLE_N), ORACLE_N, lens)])
    assert dead[0] and (kind == "tree" or dead.sum() > 1)  # (the first token; bit sets: rows of the 37-token sequence on its empty cache too)
    dead = torch.as_tensor(dead, device="cuda")
    assert (o[dead] == 0).all() and torch.equal(torch.isneginf(lse), dead[:, None].expand_as(lse)) and not torch.isnan(lse).any()


# ---- 3. the visibility probe ---------------------------------------------------------------------------------------------------------------

PROBE = [(f"{dt}_d{d}_{kind}_{layout}", dt, d, kind, layout) for dt, d in TC.PROBE_TYPES for kind in ("tree", "bits")
         for layout in (("contiguous", "paged") if dt == "f32" else ("contiguous", "paged", "fp8_paged"))]


@pytest.mark.parametrize("name,dtype,D,kind,layout", PROBE, ids=[c[0] for c in PROBE])
def test_probe_every_visible_pair_counts(name, dtype, D, kind, layout):
    comparisons, _ = TC.run_probe(dtype, D, 8, 8, kind, "cuda", page=16 if layout.endswith("paged") else 0, fp8=layout.startswith("fp8"))
    assert not VP.judge(dtype, "tree_" + name, comparisons)


@pytest.mark.parametrize("dtype,D", TC.PROBE_TYPES)
def test_probe_catches_a_single_hidden_or_leaked_bit(dtype, D):
    """the mask handed to the call differs from the expectation's in ONE bit of one row of the 64-token sequence deep in the cache (1087
    keys: the hardest row to decide): a leaked sibling, then a hidden ancestor"""
    first = sum(TC.N_B[:5])                                # packed row 0 of the sequence with N_b = 64
    words = TC.words_of("tree", TC.N_B)
    row = first + 40
    leak = next(t for t in range(40) if not (words[row] >> t) & 1)
    hide = next(t for t in range(40) if (words[row] >> t) & 1)
    for bit in (leak, hide):
        comparisons, _ = TC.run_probe(dtype, D, 8, 8, "tree", "cuda", flip=(row, bit))
        assert VP.judge(dtype, f"tree_flip_{dtype}_d{D}_bit{bit}", comparisons), f"bit {bit} of row {row} flipped and nothing noticed"


# ---- 4. graph capture -----------------------------------------------------------------------------------------------------------------------

def test_tree_step_graph_capture_and_replay():
    """One tree step with device tables, captured on a single stream and replayed after the mask, cache_seqlens and the split of total_q among
    the sequences are rewritten in place: the eager call's result and caches"""
    H, Hk, D, cap, total = 8, 2, 64, 512, 12
    q, kc, vc, kn, vn = TR._inputs("bf16", H, Hk, D, [total, 0, 0], cap, seed=4)
    cu, sl = _i32([0, 1, 4, total]), _i32([10, 300, 77])
    mask = _mask("tree", [1, 3, 8], seed=1)
    f = _api()
    kw = dict(max_seqlen_q=total, max_seqlen_k=cap, return_lse=True)
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            f(q, kc, vc, cu, kn, vn, sl, tree_mask=mask, **kw)      # warm-up (allocator, lazy init)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        kc_eager, vc_eager = kc.clone(), vc.clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out, out_lse = f(q, kc, vc, cu, kn, vn, sl, tree_mask=mask, **kw)
        for step, (table, lens, kind) in enumerate((([0, 1, 4, total], [11, 301, 78], "bits"), ([0, 6, 6, total], [12, 305, 80], "tree"),
                                                    ([0, 2, 11, total], [400, 0, 90], "chain"))):
            counts = [b - a for a, b in zip(table, table[1:])]
            q.copy_(torch.randn_like(q))
            kn.copy_(torch.randn_like(kn))
            vn.copy_(torch.randn_like(vn))
            cu.copy_(torch.tensor(table, dtype=torch.int32))
            sl.copy_(torch.tensor(lens, dtype=torch.int32))
            mask.copy_(_mask(kind, counts, seed=step))
            g.replay()
            ref, ref_lse = f(q, kc_eager, vc_eager, cu, kn, vn, sl, tree_mask=mask, **kw)
            torch.cuda.synchronize()
            assert torch.equal(out, ref) and torch.equal(out_lse, ref_lse), step
            assert torch.equal(kc, kc_eager) and torch.equal(vc, vc_eager), step
            if kind == "chain":
                causal = f(q, kc_eager, vc_eager, cu, kn, vn, sl, causal=True, **kw)
                assert torch.equal(out, causal[0]) and torch.equal(out_lse, causal[1])


# ---- 5. buffer bounds through the C ABI -------------------------------------------------------------------------------------------------------

BOUNDS = [
    # id, dtype, D, H, Hk, counts, cached, capacity, page, fp8
    ("bf16_d128_mixed", "bf16", 128, 8, 2, [1, 0, 5, 16, 37, 64, 70], [0, 17, 300, 5, 0, 1023, 200], 1200, 0, False),
    ("f32_d96_paged", "f32", 96, 4, 4, [3, 1, 0, 19, 66], [100, 0, 30, 555, 7], 640, 32, False),
    ("f16_d64_fp8_paged", "f16", 64, 8, 1, [1, 7, 33, 2], [2000, 31, 1, 4094], 4096, 16, True),
    ("bf16_d16_long_cache_splits", "bf16", 16, 2, 1, [2, 1, 9], [20000, 5, 19991], 20000 + 32, 0, False),
]


@pytest.mark.parametrize("name,dtype,D,H,Hk,counts,cached,cap,page,fp8", BOUNDS, ids=[c[0] for c in BOUNDS])
def test_tree_call_stays_inside_its_buffers(name, dtype, D, H, Hk, counts, cached, cap, page, fp8):
    """q, o, the mask, k_new, v_new, the caches, the tables and a workspace of EXACTLY fcsa_forward_kvcache_varlen_workspace_bytes (the tree
    call's formula) inside one arena pre-filled with 0xFF bytes, guard bands between them: no guard byte changes, the inputs keep their
    bits, no element of o is NaN.  Then the same call with garbage in the bits >= N_b of every word and in the words of the sequences with
    N_b > 64: the same o and lse, bit for bit."""
    from flash_cosine_sim_attention_amd import _lib
    lib = _lib.load()
    dt = DT[dtype]
    es = torch.empty((), dtype=dt).element_size()
    ces = 1 if fp8 else es
    B, total = len(counts), sum(counts)
    mb = cap // page if page else 0
    nb = B * mb + 2
    prob = _lib.problem(dt, (B, H, Hk, max(counts), cap, D), False, False, True, 1, 8.0)
    cache_elems = (nb * page if page else B * cap) * Hk * D
    kv = _lib.KvCache()
    kv.capacity, kv.page_size, kv.num_blocks, kv.new_len = cap, page, nb if page else 0, 1
    seqs = _lib.Varlen(None, None, total, 0)
    qz = _lib.KvCacheQuant() if fp8 else None
    ref = lambda x: None if x is None else C.byref(x)
    ws_n = int(lib.fcsa_forward_kvcache_varlen_workspace_bytes(C.byref(prob), C.byref(kv), C.byref(seqs), ref(qz), None))
    assert ws_n > 0
    ar = Arena((3 * total * H * D + 2 * total * Hk * D) * es + 2 * cache_elems * ces + ws_n + 8 * total + 8 * total * H
               + 4 * (B + 1 + B * max(mb, 1) + 2 * B * Hk) + 34 * (4096 + 256))
    g = torch.Generator(device="cuda").manual_seed(len(name))

    def rnd(shape, dtype_=dt):
        t = ar.take(shape, dtype_)
        t.copy_(torch.randn(shape, device="cuda", dtype=torch.float32, generator=g).to(dtype_))
        return t

    q, kn, vn = rnd((total, H, D)), rnd((total, Hk, D)), rnd((total, Hk, D))
    cshape = (nb, Hk, page, D) if page else (B, Hk, cap, D)
    if fp8:
        kc, vc = ar.take(cshape, torch.uint8), ar.take(cshape, torch.uint8)
        for c in (kc, vc):
            c.copy_(torch.randn(cshape, device="cuda", generator=g).mul(40).to(E4M3).view(torch.uint8))
        ks, vs = ar.take((B, Hk), torch.float32), ar.take((B, Hk), torch.float32)
        ks.copy_(torch.rand((B, Hk), device="cuda", generator=g) * 0.02 + 0.01)
        vs.copy_(torch.rand((B, Hk), device="cuda", generator=g) * 0.02 + 0.01)
        qz.cache_dtype, qz.k_scale, qz.v_scale = _lib.FCSA_CACHE_E4M3, ks.data_ptr(), vs.data_ptr()
        qz.k_scale_stride0, qz.k_scale_stride1, qz.v_scale_stride0, qz.v_scale_stride1 = Hk, 1, Hk, 1
    else:
        kc, vc = rnd(cshape), rnd(cshape)
    cu, sl = ar.take((B + 1,), torch.int32), ar.take((B,), torch.int32)
    cu.copy_(_cu(counts))
    sl.copy_(_i32(cached))
    if page:
        table = ar.take((B, mb), torch.int32)
        table.copy_(torch.randperm(nb, generator=torch.Generator().manual_seed(1))[:B * mb].reshape(B, mb).to(torch.int32))
        kv.block_table, kv.block_table_stride = table.data_ptr(), mb
    # the clean mask: a random tree with nothing in the bits >= N_b, zeros for the sequences of more than 64 tokens
    words = TC.words_of("tree", [n if n <= 64 else 0 for n in counts], seed=3)
    clean, at = [], 0
    for n in counts:
        clean += words[at:at + n] if n <= 64 else [0] * n
        at += n if n <= 64 else 0
    rng = np.random.default_rng(5)
    dirty, at = [], 0
    for n in counts:
        for w in clean[at:at + n]:
            junk = int(rng.integers(0, 1 << 62)) * 4 + int(rng.integers(0, 4))
            dirty.append(junk if n > 64 else w | (junk >> n << n) & ((1 << 64) - 1))
        at += n
    mask = ar.take((total,), torch.int64)
    mask.copy_(TC.as_int64(clean))
    o, o2 = ar.take((total, H, D), dt), ar.take((total, H, D), dt)
    lse, lse2 = ar.take((total, H), torch.float32), ar.take((total, H), torch.float32)
    ws = ar.take((ws_n,), torch.uint8)
    inputs = [q, kn, vn, cu, sl, mask]
    before = [t.clone() for t in inputs]
    packed = lambda t: _lib.Tensor(t.data_ptr(), 0, t.stride(1), t.stride(0))
    kv.k_cache, kv.v_cache = _lib.tensor4(kc), _lib.tensor4(vc)
    kv.k_new, kv.v_new = packed(kn), packed(vn)
    kv.cache_seqlens = sl.data_ptr()
    seqs.cu_seqlens_q = cu.data_ptr()
    none = _lib.Tensor(None, 0, 0, 0)
    tm = _lib.TreeMask(mask.data_ptr(), 0)

    def call(out, out_lse):
        fa = _lib.ForwardArgs(prob, packed(q), none, none, packed(out), None, None, None, _lib.NormState(None, None, None, None), ws.data_ptr(), ws_n,
                              torch.cuda.current_stream().cuda_stream)
        lo = _lib.LseOut(out_lse.data_ptr(), 0, out_lse.stride(1), out_lse.stride(0))
        return fa, lib.fcsa_forward_kvcache_tree(C.byref(fa), C.byref(kv), C.byref(seqs), ref(qz), C.byref(tm), C.byref(lo))

    fa, rc = call(o, lse)
    _lib.check(rc, "fcsa_forward_kvcache_tree")
    torch.cuda.synchronize()
    assert ar.guards_intact(), "a byte outside the call's buffers was written"
    for t, b in zip(inputs, before):
        assert torch.equal(t, b), "an input buffer was modified"
    bad = int((~torch.isfinite(o.float())).sum().item())
    assert bad == 0, f"o: {bad} element(s) are NaN -- never written, or computed from unwritten workspace"
    assert not torch.isnan(lse).any()
    # garbage where the rule does not look (the append writes the same rows again)
    mask.copy_(TC.as_int64(dirty))
    _, rc = call(o2, lse2)
    _lib.check(rc, "fcsa_forward_kvcache_tree")
    torch.cuda.synchronize()
    assert ar.guards_intact()
    assert torch.equal(_bits(o), _bits(o2)) and torch.equal(_bits(lse), _bits(lse2)), "bits the rule never looks at changed the result"
    # one byte less of workspace is refused, nothing launched
    fa.workspace_bytes = ws_n - 1
    lo = _lib.LseOut(lse.data_ptr(), 0, lse.stride(1), lse.stride(0))
    assert lib.fcsa_forward_kvcache_tree(C.byref(fa), C.byref(kv), C.byref(seqs), ref(qz), C.byref(tm), C.byref(lo)) == -4


def test_tree_opcheck():
    import flash_cosine_sim_attention_amd._torch_ops as ops
    ops.load()
    counts = [2, 0, 5, 1]
    q, kc, vc, kn, vn = TR._inputs("bf16", 4, 2, 32, counts, 64, seed=2)
    cu, sl, mask = _cu(counts), _i32([3, 40, 9, 63]), _mask("tree", counts)
    op = torch.ops.fcsa_tree.kvcache_tree_forward.default
    torch.library.opcheck(op, (q, kc, vc, cu, mask, kn, vn, sl, None, None, None, 5, 64, 8.0, True, 1))
    pk, pv, table = TR._paged(kc, vc, 16, seed=3)
    torch.library.opcheck(op, (q, pk, pv, cu, mask, None, None, sl, table.cuda(), None, None, 5, 64, 8.0, True, 2))
    (k8, ks), (v8, vs) = T8._quantise(kc), T8._quantise(vc)
    torch.library.opcheck(op, (q, k8.view(torch.uint8), v8.view(torch.uint8), cu, mask, kn, vn, sl, None, ks, vs, 5, 64, 8.0, True, 1))
    acc, num = _i32([[1, 2, 5], [0, 0, 0], [0, 3, 4], [0, 0, 0]]), _i32([3, 0, 2, 1])
    torch.library.opcheck(torch.ops.fcsa_tree.kvcache_compact.default, (kc, vc, _i32([3, 40, 9, 50]), acc, num, None))
    torch.library.opcheck(torch.ops.fcsa_tree.kvcache_compact.default, (pk, pv, _i32([3, 40, 9, 50]), acc, num, table.cuda()))


# ---- 6. compaction of the accepted path -----------------------------------------------------------------------------------------------------

PATHS = [list(range(64)), list(range(1, 64)), [0, 5, 6, 40, 63], [], [0, 1, 2, 5, 9]]      # identity, shift by one, scattered, none, past the capacity
COMPACT = [(f"{dt}_d{d}_hk{hk}_{'paged' if page else 'contiguous'}", dt, d, hk, page)
           for dt in ("bf16", "f32", "fp8") for d in (16, 128) for hk in (1, 8) for page in (0, 16)]


@pytest.mark.parametrize("name,dtype,D,Hk,page", COMPACT, ids=[c[0] for c in COMPACT])
def test_keep_accepted_equals_a_torch_gather(name, dtype, D, Hk, page):
    """cache_seqlens = 10 (the 64 slots cross five pages of 16); the last sequence starts 6 slots below the capacity, so its moves from or to
    the slots at or beyond it are skipped.  Bit-exact against a gather with torch on the sequence's own positions, and every byte of the
    cache (pool) outside the destination rows unchanged."""
    B, cap = len(PATHS), 96
    starts = [10, 10, 10, 10, cap - 6]
    g = torch.Generator(device="cuda").manual_seed(len(name))
    nb = B * (cap // 16) + 3
    shape = (nb, Hk, 16, D) if page else (B, Hk, cap, D)
    if dtype == "fp8":
        kc, vc = (torch.randint(0, 255, shape, device="cuda", dtype=torch.uint8, generator=g).view(E4M3) for _ in range(2))
    else:
        kc, vc = (torch.randn(shape, device="cuda", generator=g).to(DT[dtype]) for _ in range(2))
    table = None
    if page:
        table = torch.randperm(nb, generator=torch.Generator().manual_seed(7))[:B * (cap // 16)].reshape(B, cap // 16).to(torch.int32)
    where = lambda b, pos: (b, pos) if table is None else (int(table[b, pos // 16]), pos % 16)
    accepted = torch.zeros(B, 64, dtype=torch.int32)
    for b, path in enumerate(PATHS):
        accepted[b, :len(path)] = torch.tensor(path, dtype=torch.int32)
    num = [len(p) for p in PATHS]
    expect = []
    for cache in (kc, vc):
        old = _raw(cache).clone()
        new = old.clone()
        for b, path in enumerate(PATHS):
            for i, t in enumerate(path):
                if starts[b] + t < cap and starts[b] + i < cap:
                    (sb, ss), (db, ds) = where(b, starts[b] + t), where(b, starts[b] + i)
                    new[db, :, ds] = old[sb, :, ss]
        expect.append(new)
    assert _keep()(kc, vc, _i32(starts), accepted.cuda(), _i32(num), block_table=None if table is None else table.cuda()) is None
    torch.cuda.synchronize()
    assert torch.equal(_raw(kc), expect[0]) and torch.equal(_raw(vc), expect[1])


def test_keep_accepted_clamps_device_tables_and_stays_inside_its_window():
    """device tables are trusted and clamped: num_accepted to [0, A], indices to [0, 63], cache_seqlens to [0, capacity]; whatever they
    hold, nothing outside [cache_seqlens[b], cache_seqlens[b] + 64) of a sequence is written"""
    B, Hk, cap, D, guard = 3, 2, 128, 32, 4096
    n = B * Hk * cap * D
    arenas = [torch.randn(2 * guard + n, device="cuda") for _ in range(2)]
    kc, vc = (a[guard:guard + n].view(B, Hk, cap, D) for a in arenas)
    before = [a.clone() for a in arenas]
    starts = [20, 100, 500]                                # (500: clamped to the capacity, every move skipped)
    accepted = torch.tensor([[70, -3, 1000, 5], [1, 2, 3, 4], [1, 2, 3, 4]], dtype=torch.int32, device="cuda")
    assert _keep()(kc, vc, _i32(starts), accepted, _i32([9, -2, 4])) is None
    torch.cuda.synchronize()
    for a, old in zip(arenas, before):
        cache, was = a[guard:guard + n].view(B, Hk, cap, D), old[guard:guard + n].view(B, Hk, cap, D)
        assert torch.equal(a[:guard], old[:guard]) and torch.equal(a[-guard:], old[-guard:])
        inside = torch.zeros(B, cap, dtype=torch.bool, device="cuda")
        for b, s in enumerate(starts):
            inside[b, min(s, cap):min(s, cap) + 64] = True
        assert torch.equal(cache.transpose(1, 2)[~inside], was.transpose(1, 2)[~inside])
        # the clamped moves of sequence 0: 63 -> 0, 0 -> 1 (the old row), 63 -> 2, 5 -> 3
        for i, t in enumerate((63, 0, 63, 5)):
            assert torch.equal(cache[0, :, 20 + i], was[0, :, 20 + t])
        assert torch.equal(cache[1:], was[1:])             # num_accepted -2 -> 0; a start beyond the capacity


E2E = [("bf16_d64_hk2_contiguous", "bf16", 64, 2, "contiguous"), ("f16_d128_hk8_paged", "f16", 128, 8, "paged"), ("f32_d32_hk1_contiguous", "f32", 32, 1, "contiguous"),
       ("bf16_d128_hk2_fp8_paged", "bf16", 128, 2, "fp8_paged")]


@pytest.mark.parametrize("name,dtype,D,Hk,layout", E2E, ids=[c[0] for c in E2E])
def test_a_whole_speculative_step_equals_appending_only_the_accepted_tokens(name, dtype, D, Hk, layout):
    """The tree step appends every drafted token; the accepted root-to-leaf path is compacted; cache_seqlens advances by its length; then a
    plain one-token decode -- compared bit for bit (o, lse) with the same decode on caches into which only the accepted tokens were ever
    appended, in order.  One key split everywhere (capacity 240 = max_seqlen_k)."""
    H, counts, cached, cap = 8, TC.N_B, TC.BIT_CACHED, TC.BIT_CAP
    B, seed = len(counts), len(name)
    q, kc, vc, kn, vn = TR._inputs(dtype, H, Hk, D, counts, cap, seed)
    quant = {}
    if layout.startswith("fp8"):
        (kc, ks), (vc, vs) = T8._quantise(kc), T8._quantise(vc)
        kc, vc = kc.view(torch.uint8), vc.view(torch.uint8)
        quant = dict(k_scale=ks, v_scale=vs)
    table = None
    if layout.endswith("paged"):
        kc, vc, table = TR._paged(kc, vc, 16, seed)
        table = table.cuda()
    typed = (lambda t: t.view(E4M3)) if quant else (lambda t: t)
    words = TC.words_of("tree", counts, seed)
    # the accepted path of every sequence: the ancestors and self of its last token (root to leaf, strictly increasing)
    paths = [[t for t in range(n) if (own[-1] >> t) & 1] if n else [] for n, own in zip(counts, TC.split_words(words, counts))]
    A = max(len(p) for p in paths)
    accepted = torch.zeros(B, A, dtype=torch.int32)
    for b, p in enumerate(paths):
        accepted[b, :len(p)] = torch.tensor(p, dtype=torch.int32)
    num = [len(p) for p in paths]
    cu = _cu(counts, "cpu").tolist()
    common = dict(block_table=table, max_seqlen_k=cap, **quant)
    with torch.no_grad():
        # the speculative side
        ka, va = kc.clone(), vc.clone()
        _api()(q, typed(ka), typed(va), _cu(counts), kn, vn, _i32(cached), tree_mask=TC.as_int64(words, "cuda"), **common)
        _keep()(typed(ka), typed(va), _i32(cached), accepted.cuda(), _i32(num), block_table=table)
        # the side that only ever appends the accepted tokens, in order
        kb, vb = kc.clone(), vc.clone()
        rows = torch.tensor([cu[b] + t for b, p in enumerate(paths) for t in p], dtype=torch.long, device="cuda")
        _api()(q[rows], typed(kb), typed(vb), _cu(num), kn[rows], vn[rows], _i32(cached), causal=True, **common)
        # the next step: a plain decode of one token per sequence
        after = [c + n for c, n in zip(cached, num)]
        g = torch.Generator(device="cuda").manual_seed(seed + 1)
        q1 = torch.randn(B, H, D, device="cuda", generator=g).to(DT[dtype])
        k1, v1 = (torch.randn(B, Hk, D, device="cuda", generator=g).to(DT[dtype]) for _ in range(2))
        step = lambda k, v: _api()(q1, typed(k), typed(v), _cu([1] * B), k1, v1, _i32(after), causal=True, return_lse=True, **common)
        (oa, la), (ob, lb) = step(ka, va), step(kb, vb)
    torch.cuda.synchronize()
    assert torch.equal(_bits(oa), _bits(ob)) and torch.equal(_bits(la), _bits(lb))
    ksa, vsa = TK._seqs(ka, va, [n + 1 for n in after], table)
    ksb, vsb = TK._seqs(kb, vb, [n + 1 for n in after], table)
    for b in range(B):                                     # every sequence's live positions hold the same bytes
        assert torch.equal(_raw(ksa[b]), _raw(ksb[b])) and torch.equal(_raw(vsa[b]), _raw(vsb[b])), (name, b)
