"""Tree attention against MXFP4 caches on the GPU: flash_cosine_sim_attention_mxfp4_tree_with_kvcache (verify_mx_kernel) and
mxfp4_kvcache_keep_accepted (kv_compact_mx_kernel).  The reference is the float64 oracle on the DEQUANTISED caches as the call left them, with
the tree visibility as a 0 / -inf bias, under the 16-bit call's bars (tolerances.FWD_TOL with cases.logit_cond; tolerances_lse.LSE_TOL): every
cache value is exact in f16 and bf16, so the call has no tolerance of its own."""
import ctypes as C

import numpy as np
import pytest
import torch

import flash_cosine_sim_attention_amd as F
import test_gpu_kvcache as TK
import test_gpu_kvcache_mxfp4 as TM
import test_gpu_kvcache_ragged as TR
import test_gpu_kvcache_tree as TT
import tolerances_lse as TL
import tree_cases as TC

pytestmark = pytest.mark.gpu

DT, _cu, _i32, CAP = TK.DT, TR._cu, TR._i32, 1200
# Two packed batches (a batch has one G = H / Hk).  A, G = 4: one token on an EMPTY cache whose word is 0; N_b = 0; 12 rows (< 16); exactly
# 64 rows; N_b = 64 with random words (four tiles); N_b = 65 (words ignored, causal).  B, G = 3: N_b = 30, whose 90 rows put the tile
# boundary (row 64) between the heads of token 21; 15 rows.  Every P_b = cached is a multiple of neither 16, 32 nor 64.
# The two flag cases (l2norm_qk=False, groups=2) run B: those paths are per key and per row, and B is the smallest batch with whole and partial tiles.
BATCHES = {"A": (8, 2, [1, 0, 3, 16, 64, 65], [0, 17, 301, 45, 1023, 77]), "B": (6, 2, [30, 5], [333, 21])}


def _splits(dtype, D, H, Hk, counts, cap):
    """the key splits of the plan, read off the workspace query: f32 partial P~V, then (row max, row sum), of every split of every row"""
    from flash_cosine_sim_attention_amd import _lib
    total, up = sum(counts), lambda n: (n + 255) // 256 * 256
    p = _lib.problem(DT[dtype], (len(counts), H, Hk, total, cap, D))
    kv, mx, seqs = _lib.KvCache(), _lib.KvCacheMx(), _lib.Varlen()
    kv.capacity, mx.format, seqs.total_q = cap, _lib.FCSA_CACHE_MXFP4, total
    got = _lib.load().fcsa_forward_kvcache_mx_tree_workspace_bytes(C.byref(p), C.byref(kv), C.byref(mx), C.byref(seqs))
    return next(s for s in range(1, 65) if up(total * H * s * D * 4) + up(total * H * s * 8) == got)


def _inputs(dtype, D, H, Hk, counts, cap, seed, paged):
    """packed q, k_new, v_new and random MXFP4 caches (codes, codes, scales, scales), contiguous or scattered over a pool with pages of 16"""
    rnd, dt, total = TM._rnd(seed), DT[dtype], sum(counts)
    q, kn, vn = rnd(total, H, D).to(dt), rnd(total, Hk, D).to(dt), rnd(total, Hk, D).to(dt)
    mx = TM._caches(rnd, len(counts), Hk, cap, D)
    if not paged:
        return q, kn, vn, mx, None
    (kc, vc, table), (ks, vs, _) = TR._paged(mx[0], mx[1], 16, seed), TR._paged(mx[2], mx[3], 16, seed)
    return q, kn, vn, (kc, vc, ks, vs), table


def _lse_reference(q, counts, kseq, words, kw, dtype):
    """float64 log-sum-exp over the visible keys on the operands the kernel is fed, packed [total_q, H]; -inf for a row that sees none"""
    from oracle import cosine_sim_oracle as O
    cu, out = _cu(counts, "cpu").tolist(), np.full(q.shape[:2], -np.inf)
    scale, groups, l2 = kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True)
    for b, (n, own) in enumerate(zip(counts, TC.split_words(words, counts))):
        L = kseq[b].shape[1]
        if n == 0 or L == 0:
            continue
        qb, kb = TK._np(TR._rows(q, cu, b))[0], TK._np(kseq[b])
        if l2:
            qb, kb = O.rounded_operands(O.l2norm(qb, groups), O.l2norm(kb, groups), scale, dtype)
        s = np.einsum("hid,hjd->hij", qb, np.repeat(kb, q.shape[1] // kb.shape[0], axis=0)) * scale
        s = np.where(TC.visibility(own, n, L)[None], s, -np.inf)
        top = s.max(-1)
        safe = np.where(np.isfinite(top), top, 0.0)
        with np.errstate(divide="ignore"):
            out[cu[b]:cu[b + 1]] = np.where(np.isfinite(top), safe + np.log(np.exp(s - safe[..., None]).sum(-1)), -np.inf).T
    return out


ORACLE = [(f"{dt}_d{d}_{'paged' if paged else 'contiguous'}_{'AB'[(i + (i >> 1)) % 2]}", dt, d, paged, "AB"[(i + (i >> 1)) % 2], {})
          for i, (dt, d, paged) in enumerate((dt, d, pg) for dt in ("bf16", "f16") for d in (64, 128) for pg in (False, True))]
ORACLE += [("bf16_d128_no_l2norm", "bf16", 128, False, "B", dict(l2norm_qk=False, scale=0.1)), ("f16_d64_groups2", "f16", 64, True, "B", dict(groups=2))]


@pytest.mark.parametrize("name,dtype,D,paged,batch,kw", ORACLE, ids=[c[0] for c in ORACLE])
def test_random_trees_against_the_float64_oracle(name, dtype, D, paged, batch, kw):
    import cases
    H, Hk, counts, cached = BATCHES[batch]
    seed = sum(map(ord, name))
    q, kn, vn, mx, table = _inputs(dtype, D, H, Hk, counts, CAP, seed, paged)
    words = TC.words_of("tree" if seed % 2 else "bits", counts, seed)
    if batch == "A":
        words[0] = 0                                       # the one token of the empty cache sees nothing
    assert _splits(dtype, D, H, Hk, counts, CAP) > 1       # 1200 keys: several key splits at either head dimension
    with torch.no_grad():
        o, lse = F.flash_cosine_sim_attention_mxfp4_tree_with_kvcache(q, *mx, _cu(counts), kn, vn, _i32(cached), None if table is None else table.cuda(),
                                                                         return_lse=True, tree_mask=TC.as_int64(words, "cuda"), **kw)
    torch.cuda.synchronize()
    lens = [s + n for s, n in zip(cached, counts)]
    ks, vs = TK._seqs(*TM._dense(mx, DT[dtype]), lens, table)
    label = "mxfp4_tree/" + name
    cond = cases.logit_cond(dtype, kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True))
    TK._check(dtype, o, TT._reference(q, counts, ks, vs, words, kw), label + "/raw", cond)
    if kw.get("l2norm_qk", True):
        TK._check(dtype, o, TT._reference(q, counts, ks, vs, words, kw, operand_dtype=dtype), label + "/operands")
    ref, got = _lse_reference(q, counts, ks, words, kw, dtype), TK._np(lse)
    assert np.array_equal(np.isneginf(ref), np.isneginf(got)) and not np.isnan(got).any(), label
    assert np.abs(np.where(np.isinf(ref), 0.0, got - ref)).max(initial=0.0) <= TL.LSE_TOL[dtype], label
    if batch == "A":                                       # o = 0 and lse = -inf exactly
        assert (o[0] == 0).all() and torch.isneginf(lse[0]).all()


IDENTITY = [("bf16_d128_one_split", "bf16", 128, "A", 240, True), ("f16_d64_one_split_paged", "f16", 64, "B", 240, True),
            ("bf16_d64_many_splits", "bf16", 64, "A", CAP, False), ("f16_d128_many_splits_paged", "f16", 128, "B", CAP, False)]


@pytest.mark.parametrize("name,dtype,D,batch,cap,one", IDENTITY, ids=[c[0] for c in IDENTITY])
def test_chain_is_causal_and_all_ones_is_plain(name, dtype, D, batch, cap, one):
    """against flash_cosine_sim_attention_mxfp4_with_kvcache on copies of the same caches: the four cache tensors bit for bit; o and lse bit
    for bit where both calls run one key split (a 240-key cache: below two minimal splits at either head dimension), under the bars otherwise"""
    H, Hk, counts, cached = BATCHES[batch]
    counts = [n for n in counts if n <= TC.MAX_TOKENS]      # (a sequence of 65 tokens is causal under ANY mask: all ones is not causal=False there)
    cached = [min(c, cap - n) for c, n in zip(cached, counts)]
    q, kn, vn, mx, table = _inputs(dtype, D, H, Hk, counts, cap, len(name), name.endswith("paged"))
    table = None if table is None else table.cuda()
    assert (_splits(dtype, D, H, Hk, counts, cap) == 1) == one

    def run(fn, **how):
        own = [t.clone() for t in mx]
        with torch.no_grad():
            o, lse = fn(q, *own, _cu(counts), kn, vn, _i32(cached), table, return_lse=True, **how)
        return [o, lse, *own]

    for kind, causal in (("chain", True), ("full", False)):
        got = run(F.flash_cosine_sim_attention_mxfp4_tree_with_kvcache, tree_mask=TC.as_int64(TC.words_of(kind, counts), "cuda"))
        want = run(F.flash_cosine_sim_attention_mxfp4_with_kvcache, causal=causal)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got[2:], want[2:])), kind
        if one:
            assert torch.equal(TR._bits(got[0]), TR._bits(want[0])) and torch.equal(TR._bits(got[1]), TR._bits(want[1])), kind
        else:
            TK._check(dtype, got[0], TK._np(want[0]), f"mxfp4_tree/{name}/{kind}")
            assert torch.equal(torch.isneginf(got[1]), torch.isneginf(want[1]))
            assert float((got[1] - want[1]).nan_to_num(0.0, 0.0, 0.0).abs().max()) <= TL.LSE_TOL[dtype], kind


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_keep_accepted_moves_all_four_tensors(paged):
    """byte-equal to the same moves done with torch indexing on a copy: the identity path, a shift by one, a scattered path, an empty one"""
    D, Hk, cap, seq = 128, 2, 96, [3, 20, 31, 64]
    accepted = [[0, 1, 2, 3, 0], [1, 2, 3, 4, 5], [0, 5, 9, 30, 63], [7, 8, 9, 10, 11]]
    count = [4, 5, 5, 0]
    mx = TM._caches(TM._rnd(5), len(seq), Hk, cap, D)
    want = [t.clone() for t in mx]
    for b, (s, n) in enumerate(zip(seq, count)):
        for t in want:
            src = t[b, :, [s + a for a in accepted[b][:n]]].clone()
            t[b, :, s:s + n] = src
    table = None
    if paged:
        (kc, vc, table), (ks, vs, _) = TR._paged(mx[0], mx[1], 16, 3), TR._paged(mx[2], mx[3], 16, 3)
        mx = (kc, vc, ks, vs)
    F.mxfp4_kvcache_keep_accepted(*mx, _i32(seq), _i32(accepted), _i32(count), None if table is None else table.cuda())
    torch.cuda.synchronize()
    for name, got, ref in zip(("k_cache", "v_cache", "k_block_scale", "v_block_scale"), mx, want):
        if paged:
            got = torch.stack([torch.cat([got[int(i)] for i in table[b]], dim=1) for b in range(len(seq))])
        assert torch.equal(got, ref), name
