"""The 64-row verify kernel of float16 / bfloat16 / fp8 caches on the GPU: flash_cosine_sim_attention_verify_with_kvcache (verify_kernel,
fcsa_forward_kvcache_verify).  1. Random trees against the float64 oracle with the visibility as a 0 / -inf bias, under the 16-bit call's bars
(tolerances.FWD_TOL with cases.logit_cond; tolerances_lse.LSE_TOL): the kernel feeds the MFMAs what the 16-bit call feeds them, so it has no
tolerance of its own.  2. Identity with the tree call (a mask) and the ragged call (no mask, causal or not) on copies of the same caches."""
import ctypes as C

import numpy as np
import pytest
import torch

import flash_cosine_sim_attention_amd as F
import test_gpu_kvcache as TK
import test_gpu_kvcache_fp8 as T8
import test_gpu_kvcache_mxfp4_tree as TX
import test_gpu_kvcache_ragged as TR
import test_gpu_kvcache_tree as TT
import tolerances_lse as TL
import tree_cases as TC

pytestmark = pytest.mark.gpu

DT, _cu, _i32, CAP, E4M3 = TK.DT, TR._cu, TR._i32, TX.CAP, torch.float8_e4m3fn
BATCHES = TX.BATCHES      # A, G = 4: an empty cache under a word of 0, N_b = 0, 12 rows, 64 rows, four tiles, 65 tokens; B, G = 3: a tile boundary inside a token
FN = F.flash_cosine_sim_attention_verify_with_kvcache


def _splits(dtype, D, H, Hk, counts, cap, ragged=False):
    """the key splits of the plan -- ragged: of the ragged and tree calls' -- read off the workspace query: f32 partial P~V, then (row max,
    row sum), of every split of every row"""
    from flash_cosine_sim_attention_amd import _lib
    total, up = sum(counts), lambda n: (n + 255) // 256 * 256
    p = _lib.problem(DT[dtype], (len(counts), H, Hk, total, cap, D))
    kv, seqs = _lib.KvCache(), _lib.Varlen()
    kv.capacity, seqs.total_q = cap, total
    lib = _lib.load()
    got = (lib.fcsa_forward_kvcache_varlen_workspace_bytes(C.byref(p), C.byref(kv), C.byref(seqs), None, None) if ragged else
           lib.fcsa_forward_kvcache_verify_workspace_bytes(C.byref(p), C.byref(kv), C.byref(seqs), None))
    return next(s for s in range(1, 65) if up(total * H * s * D * 4) + up(total * H * s * 8) == got)


def _inputs(dtype, D, H, Hk, counts, cap, seed, paged, fp8):
    """packed q, k_new, v_new, the caches (fp8: e4m3fn codes under [B, Hk] scales other than 1), the table of a pool with pages of 16"""
    q, kc, vc, kn, vn = TR._inputs(dtype, H, Hk, D, counts, cap, seed)
    quant = {}
    if fp8:
        (kc, ks), (vc, vs) = T8._quantise(kc), T8._quantise(vc)
        kc, vc, quant = kc.view(torch.uint8), vc.view(torch.uint8), dict(k_scale=ks, v_scale=vs)
    table = None
    if paged:
        kc, vc, table = TR._paged(kc, vc, 16, seed)
    return q, kn, vn, kc, vc, table, quant


ORACLE = [(f"{dt}_d{d}_{'paged' if paged else 'contiguous'}_{'AB'[(i + (i >> 1)) % 2]}", dt, d, paged, "AB"[(i + (i >> 1)) % 2], False, {})
          for i, (dt, d, paged) in enumerate((dt, d, pg) for dt in ("bf16", "f16") for d in (64, 128) for pg in (False, True))]
ORACLE += [("bf16_d128_no_l2norm", "bf16", 128, False, "B", False, dict(l2norm_qk=False, scale=0.1)),
           ("f16_d64_groups2", "f16", 64, True, "B", False, dict(groups=2)),
           ("bf16_d128_fp8_paged", "bf16", 128, True, "A", True, {}), ("f16_d64_fp8_contiguous", "f16", 64, False, "B", True, {})]


@pytest.mark.parametrize("name,dtype,D,paged,batch,fp8,kw", ORACLE, ids=[c[0] for c in ORACLE])
def test_random_trees_against_the_float64_oracle(name, dtype, D, paged, batch, fp8, kw):
    import cases
    H, Hk, counts, cached = BATCHES[batch]
    seed = sum(map(ord, name))
    q, kn, vn, kc, vc, table, quant = _inputs(dtype, D, H, Hk, counts, CAP, seed, paged, fp8)
    typed = (lambda t: t.view(E4M3)) if fp8 else (lambda t: t)
    words = TC.words_of("tree" if seed % 2 else "bits", counts, seed)
    if batch == "A":
        words[0] = 0                                       # the one token of the empty cache sees nothing
    assert _splits(dtype, D, H, Hk, counts, CAP) > 1       # 1200 keys: several key splits at either head dimension
    with torch.no_grad():
        o, lse = FN(q, typed(kc), typed(vc), _cu(counts), kn, vn, _i32(cached), None if table is None else table.cuda(), return_lse=True,
                    tree_mask=TC.as_int64(words, "cuda"), **quant, **kw)
    torch.cuda.synchronize()
    lens = [s + n for s, n in zip(cached, counts)]
    ks, vs = T8._seqs(kc, vc, quant["k_scale"], quant["v_scale"], lens, table) if fp8 else TK._seqs(kc, vc, lens, table)      # fp8: scale * code
    label = "verify/" + name
    cond = cases.logit_cond(dtype, kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True))
    TK._check(dtype, o, TT._reference(q, counts, ks, vs, words, kw), label + "/raw", cond)
    if kw.get("l2norm_qk", True):
        TK._check(dtype, o, TT._reference(q, counts, ks, vs, words, kw, operand_dtype=dtype), label + "/operands")
    ref, got = TX._lse_reference(q, counts, ks, words, kw, dtype), TK._np(lse)
    assert np.array_equal(np.isneginf(ref), np.isneginf(got)) and not np.isnan(got).any(), label
    assert np.abs(np.where(np.isinf(ref), 0.0, got - ref)).max(initial=0.0) <= TL.LSE_TOL[dtype], label
    if batch == "A":                                       # o = 0 and lse = -inf exactly
        assert (o[0] == 0).all() and torch.isneginf(lse[0]).all()


IDENTITY = [("bf16_d128_one_split", "bf16", 128, "A", 240, False), ("f16_d64_fp8_one_split_paged", "f16", 64, "B", 240, True),
            ("f16_d64_many_splits_paged", "f16", 64, "A", CAP, False), ("bf16_d128_fp8_many_splits", "bf16", 128, "B", CAP, True)]


@pytest.mark.parametrize("name,dtype,D,batch,cap,fp8", IDENTITY, ids=[c[0] for c in IDENTITY])
def test_equals_the_tree_call_and_the_ragged_call(name, dtype, D, batch, cap, fp8):
    """on copies of the same caches: the caches after the append bit for bit; o and lse bit for bit where both calls plan one key split (a
    240-key cache: below two minimal splits at either head dimension), under the bars of the oracle test and with lse's -inf pattern otherwise"""
    H, Hk, counts, cached = BATCHES[batch]
    cached = [min(c, cap - n) for c, n in zip(cached, counts)]
    q, kn, vn, kc, vc, table, quant = _inputs(dtype, D, H, Hk, counts, cap, len(name), name.endswith("paged"), fp8)
    table = None if table is None else table.cuda()
    typed = (lambda t: t.view(E4M3)) if fp8 else (lambda t: t)
    one = cap == 240
    assert (_splits(dtype, D, H, Hk, counts, cap) == 1) == one and (_splits(dtype, D, H, Hk, counts, cap, ragged=True) == 1) == one

    def run(fn, **how):
        k, v = kc.clone(), vc.clone()
        with torch.no_grad():
            o, lse = fn(q, typed(k), typed(v), _cu(counts), kn, vn, _i32(cached), table, return_lse=True, max_seqlen_k=cap, **quant, **how)
        return o, lse, k, v

    mask = TC.as_int64(TC.words_of("tree", counts, len(name)), "cuda")
    ragged = F.flash_cosine_sim_attention_varlen_with_kvcache
    for kind, other, how in (("tree", F.flash_cosine_sim_attention_tree_with_kvcache, dict(tree_mask=mask)), ("causal", ragged, dict(causal=True)),
                             ("full", ragged, dict(causal=False))):
        got, want = run(FN, **how), run(other, **how)
        torch.cuda.synchronize()
        assert torch.equal(TR._bits(got[2]), TR._bits(want[2])) and torch.equal(TR._bits(got[3]), TR._bits(want[3])), kind      # (spare pages hold NaN)
        if one:
            assert torch.equal(TR._bits(got[0]), TR._bits(want[0])) and torch.equal(TR._bits(got[1]), TR._bits(want[1])), kind
        else:
            TK._check(dtype, got[0], TK._np(want[0]), f"verify/{name}/{kind}")
            assert torch.equal(torch.isneginf(got[1]), torch.isneginf(want[1])) and not torch.isnan(got[1]).any(), kind
            assert float((got[1] - want[1]).nan_to_num(0.0, 0.0, 0.0).abs().max()) <= TL.LSE_TOL[dtype], kind
