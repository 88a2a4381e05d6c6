"""flash_cosine_sim_attention_rotary_with_kvcache on the GPU against float64: q and k_new rotated with numpy from the same float32 tables
(tests/rotary_reference.py), the rotated k_new put into a float64 copy of each sequence's cache (an fp8 cache keeps its own codes: the append
is judged in test_what_the_append_wrote), the oracle per sequence.  The operand-faithful pass is fed what the kernel's S product is fed: q
rotated in float32 as the kernel rotates it, the keys as the cache holds them.  Bars: the existing ones.  Shapes: the ALiBi file's."""
import numpy as np
import pytest
import torch

import flash_cosine_sim_attention_amd as F
import test_gpu_kvcache as TK
import test_gpu_kvcache_alibi as TA
import test_gpu_kvcache_fp8 as T8
import test_gpu_kvcache_ragged as TR
import tolerances as T
from rotary_reference import rotate, tables

pytestmark = pytest.mark.gpu
_cu, _i32, _bits, _np = TR._cu, TR._i32, TR._bits, TK._np
COUNTS, CACHED, CAP, H, HK = TA.COUNTS, TA.CACHED, TA.CAP, TA.H, TA.HK
E4M3 = torch.float8_e4m3fn


def positions(counts, cached, cap, append):
    """(query positions L_b - N_b + i, append slots cache_seqlens[b] + i), packed"""
    qp = [min(s + (n if append else 0), cap) - n + i for n, s in zip(counts, cached) for i in range(n)]
    return qp, [s + i for n, s in zip(counts, cached) for i in range(n)]


def _reference(qr, kseq, vseq, kw, operand_dtype=None):
    """float64 (o, lse): the ALiBi file's reference at zero slopes (its eps of 1e-300 serves both regimes: no row sum is near the static clamp)"""
    return TA._reference(torch.from_numpy(qr), COUNTS, kseq, vseq, kw, torch.zeros(H), operand_dtype, with_lse=True)


def _run(dtype, D, rotary_dim, interleaved, chunk_rows, cached=CACHED, append=True, fp8=False, seed=0, random=False, rows=CAP, **kw):
    """One call on fresh inputs: o, lse, q rotated in (float64, float32), K as (float64-rotated k_new appended, the cache holds it), V"""
    q, kc, vc, kn, vn = TR._inputs(dtype, H, HK, D, COUNTS, CAP, seed, append)
    if not kw.get("l2norm_qk", True):
        (q, kc), (_, kn) = TK._unit_normalised(q, kc, 1, False), TK._unit_normalised(q, kn, 1, False)
    cos, sin = tables(rows, rotary_dim, random)
    quant, ks, vs = {}, None, None
    if fp8:
        (kc, ks), (vc, vs) = T8._quantise(kc), T8._quantise(vc)
        ks, vs = ks[0].contiguous() * 1.5, vs[1].contiguous() * 0.75      # per K/V head
        quant = dict(k_scale=ks, v_scale=vs)
    with torch.no_grad():
        o, lse = F.flash_cosine_sim_attention_rotary_with_kvcache(
            q, kc, vc, _cu(COUNTS), kn, vn, _i32(cached), max_seqlen_k=CAP, return_lse=True, chunk_rows=chunk_rows, rotary_cos=cos.cuda(),
            rotary_sin=sin.cuda(), rotary_interleaved=interleaved, **quant, **kw)
    torch.cuda.synchronize()
    assert o.shape == q.shape and o.dtype == q.dtype and lse.shape == q.shape[:2] and lse.dtype == torch.float32
    lens = [min(s + (n if append else 0), CAP) for s, n in zip(cached, COUNTS)]
    kseq, vseq = T8._seqs(kc, vc, ks, vs, lens) if fp8 else TK._seqs(kc, vc, lens)
    held, vseq = [_np(x) for x in kseq], [_np(x) for x in vseq]
    kseq, (qp, kp) = [x.copy() for x in held], positions(COUNTS, cached, CAP, append)
    if append and not fp8:
        kr, cu = rotate(kn, kp, cos, sin, interleaved)[0], _cu(COUNTS, "cpu").tolist()
        for b, (s, n) in enumerate(zip(cached, COUNTS)):
            kseq[b][:, s:s + n] = kr[cu[b]:cu[b + 1]].transpose(1, 0, 2)
    return o, lse, (rotate(q, qp, cos, sin, interleaved)[0], rotate(q, qp, cos, sin, interleaved, float32=True)[0]), (kseq, held), vseq


def _verify(dtype, o, lse, qr, kseq, vseq, kw, label):
    """the existing bars of o (TR._verify's policy) and of lse (the ALiBi file's): the raw pass, and with l2norm the operand-faithful one"""
    import cases
    import lse_reference as R
    import tolerances_lse as TL
    scale, groups, l2 = kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True)
    ref_o, ref_l = _reference(qr[0], kseq[0], vseq, kw)
    TK._check(dtype, o, ref_o, label + "/raw", cases.logit_cond(dtype, scale, groups, l2))
    seen, got = np.isfinite(ref_l), _np(lse)
    assert (np.isneginf(got) == ~seen).all(), label
    d_raw = float(np.abs(got - ref_l)[seen].max())
    assert T.check(label + "/lse-raw", dtype, d_raw, R.derived_lse_bound(dtype, scale, groups, l2)), d_raw
    if l2:
        ops_o, ops_l = _reference(qr[1], kseq[1], vseq, kw, operand_dtype=dtype)
        TK._check(dtype, o, ops_o, label + "/operands")
        d_ops = float(np.abs(got - ops_l)[seen].max())
        assert T.check(label + "/lse-operands", dtype, d_ops, TL.LSE_TOL[dtype]), d_ops


@pytest.mark.parametrize("dtype,D,rotary_dim", [("bf16", 128, 128), ("f16", 64, 64), ("bf16", 128, 64)])
@pytest.mark.parametrize("interleaved", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("route,chunk_rows", TA.ROUTES, ids=[r[0] for r in TA.ROUTES])
def test_parity(dtype, D, rotary_dim, interleaved, route, chunk_rows):
    if chunk_rows != TA.ALL_CHUNK:
        TA._splits_above_one(dtype, len(COUNTS), H, HK, D, sum(COUNTS), CAP, 0, True, True, chunk_rows)
    o, lse, qr, ks, vs = _run(dtype, D, rotary_dim, interleaved, chunk_rows, causal=True, seed=D + rotary_dim)
    _verify(dtype, o, lse, qr, ks, vs, dict(causal=True), f"rotary/{dtype}/{D}/{rotary_dim}/{route}/{int(interleaved)}")


@pytest.mark.parametrize("interleaved", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("page", [0, 16], ids=["contiguous", "pages16"])
@pytest.mark.parametrize("dtype,D,rotary_dim", [("bf16", 128, 64), ("f16", 64, 64), ("bf16", 128, 128)])
def test_what_the_append_wrote(dtype, D, rotary_dim, page, fp8, interleaved):
    """Every appended K element against the float64 rotation r of (x, y): one unit in the last place of the cache type (bf16 2^-8 |r|; f16
    2^-11 |r| + 2^-24; fp8 2^-4 |r| + 2^-10 k_scale, k_scale = 1.01 sqrt(2) amax / 448: nothing clamps) plus 2^-21 (|x| + |y|) for float32
    under cancellation.  V, untouched slots, rows beyond the capacity (sequence 0 keeps 3 of 7), pass-through features: the step call's bytes."""
    counts, cached, cap = [7, 0, 19, 1], [125, 5, 40, 0], 128
    q, kc, vc, kn, vn = TR._inputs(dtype, H, HK, D, counts, cap, 3 + page + D)
    cos, sin = tables(cap, rotary_dim, random=True)
    quant, scale = {}, 2 ** 0.5 * float(kn.float().abs().max()) / 448 * 1.01
    if fp8:
        quant = dict(k_scale=torch.full((HK,), scale, device="cuda"), v_scale=torch.full((HK,), 0.02, device="cuda"))
        kc, vc = ((t.float().clamp(-3, 3) * 20).to(E4M3).view(torch.uint8) for t in (kc, vc))      # any codes: the cache's old content
    table = None
    if page:
        kc, vc, table = TR._paged(kc, vc, page, 11)
    typed = (lambda t: t.view(E4M3)) if fp8 else (lambda t: t)
    k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    args = dict(block_table=None if table is None else table.cuda(), causal=True, chunk_rows=TA.MIXED, **quant)
    with torch.no_grad():
        F.flash_cosine_sim_attention_rotary_with_kvcache(q, typed(k1), typed(v1), _cu(counts), kn, vn, _i32(cached), rotary_cos=cos.cuda(),
                                                            rotary_sin=sin.cuda(), rotary_interleaved=interleaved, **args)
        F.flash_cosine_sim_attention_step_with_kvcache(q, typed(k2), typed(v2), _cu(counts), kn, vn, _i32(cached), **args)
    torch.cuda.synchronize()
    assert torch.equal(_bits(v1), _bits(v2))
    r, mag = rotate(kn, positions(counts, cached, cap, True)[1], cos, sin, interleaved)      # [total, Hk, D]
    lens, cu = [cap] * len(counts), _cu(counts, "cpu").tolist()
    raw, plain, before = (TK._seqs(k, v1, lens, table)[0] for k in (k1, k2, kc))
    value = T8._seqs(k1, v1, scale, 1.0, lens, table)[0] if fp8 else raw
    ulp = {"bf16": (2.0 ** -8, 0.0), "f16": (2.0 ** -11, 2.0 ** -24)}[dtype] if not fp8 else (2.0 ** -4, 2.0 ** -10 * scale)
    for b, (s, n) in enumerate(zip(cached, counts)):
        kept = max(min(s + n, cap) - s, 0)
        got, want = _np(value[b])[:, s:s + kept].transpose(1, 0, 2), r[cu[b]:cu[b] + kept]
        bound = ulp[0] * np.abs(want) + ulp[1] + 2.0 ** -21 * mag[cu[b]:cu[b] + kept]
        assert (np.abs(got - want) <= bound).all(), (b, float((np.abs(got - want) - bound).max()))
        untouched = torch.ones(cap, dtype=torch.bool)
        untouched[s:s + kept] = False
        assert torch.equal(_bits(raw[b][:, untouched]), _bits(before[b][:, untouched])), b
        assert torch.equal(_bits(raw[b][:, :, rotary_dim:]), _bits(plain[b][:, :, rotary_dim:])), b


VARIANTS = [
    ("window_33_0_causal", "f16", 64, 64, False, dict(kw=dict(causal=True, window_size=(33, 0)))),
    ("noncausal", "bf16", 128, 128, True, dict(kw=dict(causal=False))),
    ("groups_2", "bf16", 128, 64, False, dict(kw=dict(causal=True, groups=2))),
    ("raw_qk", "f16", 128, 128, False, dict(kw=dict(causal=True, l2norm_qk=False, scale=4.0))),
    ("no_append", "bf16", 128, 128, True, dict(append=False, kw=dict(causal=True))),
    ("fp8_per_head", "bf16", 128, 64, False, dict(fp8=True, kw=dict(causal=True))),
    ("random_angles", "f16", 64, 64, True, dict(random=True, kw=dict(causal=True))),
    ("short_table_mixed", "bf16", 128, 128, False, dict(rows=600, kw=dict(causal=True))),      # device positions up to 1059: row 599, as the reference clamps
    ("short_table_decode", "bf16", 128, 128, False, dict(rows=600, chunk_rows=TA.ALL_DECODE, kw=dict(causal=True))),
]


@pytest.mark.parametrize("name,dtype,D,rotary_dim,interleaved,opt", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_parity_variants(name, dtype, D, rotary_dim, interleaved, opt):
    append = opt.get("append", True)
    cached = CACHED if append else [1060, 300, 17, 1060, 3, 640]      # every query keeps a visible key without the append
    o, lse, qr, ks, vs = _run(dtype, D, rotary_dim, interleaved, opt.get("chunk_rows", TA.MIXED), cached=cached, append=append,
                              fp8=opt.get("fp8", False), random=opt.get("random", False), rows=opt.get("rows", CAP), seed=len(name), **opt["kw"])
    _verify(dtype, o, lse, qr, ks, vs, opt["kw"], "rotary/" + name)


@pytest.mark.parametrize("chunk_rows", [TA.MIXED, TA.ALL_DECODE], ids=["mixed", "decode"])
def test_identities(chunk_rows):
    """cos = 1, sin = 0 is the step call; a sequence in a batch equals the sequence alone (one key split, as in the ALiBi file): bit for bit"""
    q, kc, vc, kn, vn = TR._inputs("bf16", H, HK, 128, COUNTS, CAP, 5)
    cu, rot = _cu(COUNTS, "cpu").tolist(), F.flash_cosine_sim_attention_rotary_with_kvcache
    kw = dict(return_lse=True, causal=True, chunk_rows=chunk_rows)
    one, zero = torch.ones(CAP, 64, device="cuda"), torch.zeros(CAP, 64, device="cuda")
    tab = dict(zip(("rotary_cos", "rotary_sin"), (t.cuda() for t in tables(CAP, 128))), max_seqlen_k=1)
    eq = lambda *pairs: all(torch.equal(_bits(a), _bits(b)) for a, b in pairs)
    with torch.no_grad():
        k1, v1, k2, v2, k3 = kc.clone(), vc.clone(), kc.clone(), vc.clone(), kc.clone()
        o1, l1 = rot(q, k1, v1, _cu(COUNTS), kn, vn, _i32(CACHED), rotary_cos=one, rotary_sin=zero, **kw)
        o2, l2 = F.flash_cosine_sim_attention_step_with_kvcache(q, k2, v2, _cu(COUNTS), kn, vn, _i32(CACHED), **kw)
        assert eq((o1, o2), (l1, l2), (k1, k2), (v1, v2))
        o, lse = rot(q, k3, vc.clone(), _cu(COUNTS), kn, vn, _i32(CACHED), **tab, **kw)
        for b, n in enumerate(COUNTS):
            if n:
                kb, rows = kc[b:b + 1].clone(), slice(cu[b], cu[b + 1])
                ob, lb = rot(q[rows], kb, vc[b:b + 1].clone(), _cu([n]), kn[rows], vn[rows], _i32([CACHED[b]]), **tab, **kw)
                assert eq((o[rows], ob), (lse[rows], lb), (k3[b:b + 1], kb)), b
