"""The linear position bias of the cached calls on the GPU (flash_cosine_sim_attention_alibi_with_kvcache, fcsa_forward_kvcache_alibi): the
engine step with per-head slopes, the logit of key j gaining -slope[b, h] * |L_b - N_b + i - j|.

The reference is the float64 oracle per sequence with attn_bias = band + ALiBi matrix and eps = 1e-300 (every call with slopes runs the
per-row-shift regime), as test_gpu_kvcache_ragged._reference builds its window reference; the bars are the existing FWD_TOL under
test_gpu_kvcache._check (raw pass scaled by cases.logit_cond, operand-faithful pass fixed) and the existing lse bars.  Shapes are the
smallest that reach each path: counts [1, 5, 0, 40, 1, 17] with H 8 / Hk 2 put sequences on both sides of chunk_rows = 64, cached lengths
up to 1060 of a capacity of 1152 give the decode side several key splits (asserted from the workspace query)."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_kvcache as TK
import test_gpu_kvcache_fp8 as T8
import test_gpu_kvcache_ragged as TR
import tolerances as T
from test_gpu_window import band

pytestmark = pytest.mark.gpu

DT = TK.DT
_cu, _i32, _bits, _paged, _np = TR._cu, TR._i32, TR._bits, TR._paged, TK._np
COUNTS = [1, 5, 0, 40, 1, 17]
CACHED = [1059, 300, 17, 1020, 0, 640]
CAP = 1152
H, HK = 8, 2
ALL_DECODE, ALL_CHUNK, MIXED = 10 ** 9, 0, 64
E4M3 = torch.float8_e4m3fn


def _F():
    import flash_cosine_sim_attention_amd as F
    return F


def _alibi(*a, **kw):
    return _F().flash_cosine_sim_attention_alibi_with_kvcache(*a, **kw)


def std_slopes(heads):
    return torch.tensor([2.0 ** (-8.0 * (h + 1) / heads) for h in range(heads)], dtype=torch.float32)


def alibi_matrix(slopes, n, L):
    """[H, n, L] float64: -slope_h * |L - n + i - j|"""
    i = np.arange(n)[:, None] + (L - n)
    j = np.arange(L)[None]
    return -np.asarray(slopes, np.float64)[:, None, None] * np.abs(i - j)[None]


def _reference(q, counts, kseq, vseq, kw, slopes, operand_dtype=None, with_lse=False):
    """float64 o (packed like q) and lse [total, H] of every sequence; slopes: float32 tensor [H] or [B, H]"""
    from oracle import cosine_sim_oracle as O
    cu = _cu(counts, "cpu").tolist()
    out, lse = np.zeros(q.shape), np.full(q.shape[:2], -np.inf)
    scale, groups, l2, causal = kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True), kw.get("causal", False)
    left, right = kw.get("window_size", (-1, -1))
    sl = slopes.detach().cpu().double().numpy()
    for b, n in enumerate(counts):
        L = kseq[b].shape[1]
        if n == 0 or L == 0:
            continue
        qb = _np(TR._rows(q, cu, b))
        G = q.shape[1] // kseq[b].shape[0]
        kr, vr = (np.repeat((_np(x) if isinstance(x, torch.Tensor) else x)[None], G, axis=1) for x in (kseq[b], vseq[b]))
        bias = band(n, L, left, right, causal) + alibi_matrix(sl if sl.ndim == 1 else sl[b], n, L)
        o = O.attention_forward_stats(qb, kr, vr, scale=scale, groups=groups, causal=causal, l2norm_qk=l2, attn_bias=bias, eps=1e-300,
                                      operand_dtype=operand_dtype)[0]
        out[cu[b]:cu[b + 1]] = o[0].transpose(1, 0, 2)
        if with_lse:
            qn, kn = qb, kr
            if l2:      # lse_reference.lse_rows' operands: c1 * q^ and k^ rounded to the type the S product is fed
                qn, kn = O.rounded_operands(O.l2norm(qb, groups), O.l2norm(kr, groups), scale, operand_dtype)
            s = scale * np.einsum("bhid,bhjd->bhij", qn, kn)[0] + bias
            m = s.max(axis=-1, keepdims=True)
            ms = np.where(np.isneginf(m), 0.0, m)
            tot = np.exp(s - ms).sum(axis=-1)
            with np.errstate(divide="ignore"):
                lse[cu[b]:cu[b + 1]] = (ms[..., 0] + np.log(tot)).T
    return (out, lse) if with_lse else out


def _verify(dtype, o, q, counts, kseq, vseq, kw, slopes, label):
    """test_gpu_kvcache_ragged._verify's policy with the bias in the reference: the existing bars, unchanged"""
    import cases
    cond = cases.logit_cond(dtype, kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True))
    TK._check(dtype, o, _reference(q, counts, kseq, vseq, kw, slopes), label + "/raw", cond)
    if dtype != "f32" and kw.get("l2norm_qk", True):
        TK._check(dtype, o, _reference(q, counts, kseq, vseq, kw, slopes, operand_dtype=dtype), label + "/operands")


def _splits_above_one(dtype, B, heads, hk, D, total, capacity, page, causal, append, chunk_rows):
    """the step's workspace for these bounds holds more than one split of partials"""
    from flash_cosine_sim_attention_amd import _lib
    lib = _lib.load()
    prob = _lib.problem(DT[dtype], (B, heads, hk, total, capacity, D), causal, False, True, 1, 8.0)
    kv = _lib.KvCache()
    kv.capacity, kv.page_size, kv.num_blocks, kv.new_len = capacity, page, (B * (capacity // page) if page else 0), int(append)
    seqs = _lib.Varlen(None, None, total, 0)
    st = _lib.KvCacheStep(min(chunk_rows, 2 ** 31 - 1), 0, -1, 0, 0)
    got = int(lib.fcsa_forward_kvcache_step_workspace_bytes(C.byref(prob), C.byref(kv), C.byref(seqs), None, None, C.byref(st)))
    one = (total * heads * D * 4 + 255) // 256 * 256 + (total * heads * 8 + 255) // 256 * 256
    assert got > one, (got, one)


def _run(dtype, D, counts, cached, cap, slopes, chunk_rows, heads=H, hk=HK, page=0, append=True, fp8=False, seed=0, max_k=None, **kw):
    """one call on fresh inputs; returns (o, lse, q, kseq, vseq) with the sequences as the kernel saw them (after the append)"""
    q, kc, vc, kn, vn = TR._inputs(dtype, heads, hk, D, counts, cap, seed, append)
    if not kw.get("l2norm_qk", True):
        q, kc = TK._unit_normalised(q, kc, 1, False)
        if kn is not None:
            _, kn = TK._unit_normalised(q, kn, 1, False)
    quant, ks, vs = {}, None, None
    if fp8:
        (kc, ks), (vc, vs) = T8._quantise(kc), T8._quantise(vc)
        ks, vs = ks[0].contiguous() * 1.25, vs[1].contiguous() * 0.75      # per K/V head
        kc, vc = kc.view(torch.uint8), vc.view(torch.uint8)
        quant = dict(k_scale=ks, v_scale=vs)
    table = None
    if page:
        kc, vc, table = _paged(kc, vc, page, seed)
    typed = (lambda t: t.view(E4M3)) if fp8 else (lambda t: t)
    with torch.no_grad():
        o, lse = _alibi(q, typed(kc), typed(vc), _cu(counts), kn, vn, _i32(cached), block_table=None if table is None else table.cuda(),
                        max_seqlen_k=cap if max_k is None else max_k, return_lse=True, chunk_rows=chunk_rows,
                        alibi_slopes=slopes.cuda(), **quant, **kw)
    torch.cuda.synchronize()
    assert o.shape == q.shape and o.dtype == q.dtype and lse.shape == q.shape[:2] and lse.dtype == torch.float32
    lens = [min(s + (n if append else 0), cap) for s, n in zip(cached, counts)]
    if fp8:
        kseq, vseq = T8._seqs(kc, vc, ks, vs, lens, table)
    else:
        kseq, vseq = TK._seqs(kc, vc, lens, table)
    return o, lse, q, kseq, vseq


ROUTES = [("decode", ALL_DECODE), ("chunk", ALL_CHUNK), ("mixed", MIXED)]


# ---- 1. parity over the three routings --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", [("bf16", 128), ("f16", 64)])
@pytest.mark.parametrize("route,chunk_rows", ROUTES, ids=[r[0] for r in ROUTES])
def test_parity_over_routings(dtype, D, route, chunk_rows):
    slopes = std_slopes(H)
    if chunk_rows != ALL_CHUNK:
        _splits_above_one(dtype, len(COUNTS), H, HK, D, sum(COUNTS), CAP, 0, True, True, chunk_rows)
    o, lse, q, ks, vs = _run(dtype, D, COUNTS, CACHED, CAP, slopes, chunk_rows, causal=True, seed=D)
    _verify(dtype, o, q, COUNTS, ks, vs, dict(causal=True), slopes, f"alibi/{dtype}/{route}")


# ---- 2. one case each of what composes with the bias ------------------------------------------------------------------------------------
VARIANTS = [
    ("noncausal", "bf16", 128, dict(kw=dict(causal=False))),
    ("window_33_0_causal", "f16", 64, dict(kw=dict(causal=True, window_size=(33, 0)))),
    ("window_70_5", "bf16", 128, dict(kw=dict(causal=False, window_size=(70, 5)))),
    ("fp8_per_head", "bf16", 128, dict(fp8=True, kw=dict(causal=True))),
    ("pages_of_16", "f16", 64, dict(page=16, kw=dict(causal=True))),
    ("groups_2", "bf16", 64, dict(kw=dict(causal=True, groups=2))),
    ("raw_qk", "f16", 128, dict(kw=dict(causal=True, l2norm_qk=False, scale=4.0))),
    ("f32_d32", "f32", 32, dict(kw=dict(causal=True))),
    ("bf16_d96", "bf16", 96, dict(kw=dict(causal=True))),
    ("no_append", "bf16", 128, dict(append=False, kw=dict(causal=True))),
]


@pytest.mark.parametrize("name,dtype,D,opt", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_parity_variants(name, dtype, D, opt):
    slopes = std_slopes(H)
    kw = opt["kw"]
    cached = CACHED if opt.get("append", True) else [1060, 300, 17, 1060, 3, 640]      # every query keeps a visible key without the append
    o, lse, q, ks, vs = _run(dtype, D, COUNTS, cached, CAP, slopes, MIXED, page=opt.get("page", 0), append=opt.get("append", True),
                             fp8=opt.get("fp8", False), seed=len(name), **kw)
    _verify(dtype, o, q, COUNTS, ks, vs, kw, slopes, "alibi/" + name)


@pytest.mark.parametrize("chunk_rows", [MIXED, ALL_DECODE], ids=["mixed", "decode"])
@pytest.mark.parametrize("form", ["H", "BH"])
def test_a_sequence_inside_a_batch_equals_the_sequence_alone(form, chunk_rows):
    """[H] slopes, and [B, H] slopes against each sequence's own [H] row: every sequence of the batch equals the call on that sequence
    alone, bit for bit.  At one key split on both sides (max_seqlen_k = 1): the split count is planned from the batch's row tiles, so a
    batch and a single sequence at real bounds need not run the same count, and partials summed in another order round differently --
    several splits are judged against the oracle in test_parity_over_routings."""
    dtype, D = "bf16", 128
    B = len(COUNTS)
    slopes = std_slopes(H)
    if form == "BH":
        slopes = (slopes[None] * (1 + torch.arange(B, dtype=torch.float32)[:, None] / 4)).contiguous()
    q, kc, vc, kn, vn = TR._inputs(dtype, H, HK, D, COUNTS, CAP, 5)
    cu = _cu(COUNTS, "cpu").tolist()
    kw = dict(max_seqlen_k=1, return_lse=True, causal=True, chunk_rows=chunk_rows)
    with torch.no_grad():
        o, lse = _alibi(q, kc.clone(), vc.clone(), _cu(COUNTS), kn, vn, _i32(CACHED), alibi_slopes=slopes.cuda(), **kw)
        for b, n in enumerate(COUNTS):
            if n == 0:
                continue
            mine = slopes if form == "H" else slopes[b]
            ob, lb = _alibi(q[cu[b]:cu[b + 1]], kc[b:b + 1].clone(), vc[b:b + 1].clone(), _cu([n]), kn[cu[b]:cu[b + 1]], vn[cu[b]:cu[b + 1]],
                            _i32([CACHED[b]]), alibi_slopes=mine.cuda(), **kw)
            assert torch.equal(_bits(o[cu[b]:cu[b + 1]]), _bits(ob)) and torch.equal(_bits(lse[cu[b]:cu[b + 1]]), _bits(lb)), b


# ---- 3. identities, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", [("bf16", 128), ("f16", 64)])
def test_chunk_kernel_equals_decode_kernel_at_one_split(dtype, D):
    slopes = std_slopes(H).cuda()
    q, kc, vc, kn, vn = TR._inputs(dtype, H, HK, D, COUNTS, CAP, 11)
    res = []
    for chunk_rows in (ALL_CHUNK, ALL_DECODE):
        k2, v2 = kc.clone(), vc.clone()
        with torch.no_grad():
            o, lse = _alibi(q, k2, v2, _cu(COUNTS), kn, vn, _i32(CACHED), max_seqlen_k=1, return_lse=True, causal=True, chunk_rows=chunk_rows,
                            alibi_slopes=slopes)
        res.append((o, lse, k2, v2))
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(res[0][2]), _bits(TR._appended(kc, kn, COUNTS, CACHED)))


@pytest.mark.parametrize("chunk_rows", [ALL_DECODE, ALL_CHUNK])
def test_zero_slopes_equal_the_step_call_in_the_per_row_regime(chunk_rows):
    """f16 at scale 16 runs the per-row shift in the step call too: zero slopes give its bits"""
    import cases
    assert cases.dynamic_shift_regime("f16", 16.0, 1, True, False)
    q, kc, vc, kn, vn = TR._inputs("f16", H, HK, 64, COUNTS, CAP, 13)
    kw = dict(max_seqlen_k=CAP, return_lse=True, causal=True, chunk_rows=chunk_rows, scale=16.0)
    with torch.no_grad():
        o, lse = _alibi(q, kc.clone(), vc.clone(), _cu(COUNTS), kn, vn, _i32(CACHED), alibi_slopes=torch.zeros(H, device="cuda"), **kw)
        o_ref, lse_ref = _F().flash_cosine_sim_attention_step_with_kvcache(q, kc.clone(), vc.clone(), _cu(COUNTS), kn, vn, _i32(CACHED), **kw)
    assert torch.equal(_bits(o), _bits(o_ref)) and torch.equal(_bits(lse), _bits(lse_ref))


def test_zero_slopes_elsewhere_are_within_the_bars():
    slopes = torch.zeros(H)
    o, lse, q, ks, vs = _run("bf16", 128, COUNTS, CACHED, CAP, slopes, MIXED, causal=True, seed=17)
    assert not cases_dyn("bf16")
    TR._verify("bf16", o, q, COUNTS, ks, vs, dict(causal=True), "alibi/zero")


def cases_dyn(dtype):
    import cases
    return cases.dynamic_shift_regime(dtype, 8.0, 1, True, False)


# ---- 4. the regime: a negative slope and a steep one ------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,chunk_rows", ROUTES, ids=[r[0] for r in ROUTES])
def test_negative_and_steep_slopes(route, chunk_rows):
    slopes = std_slopes(H)
    slopes[1], slopes[6] = -0.25, 50.0
    o, lse, q, ks, vs = _run("f16", 64, COUNTS, CACHED, CAP, slopes, chunk_rows, causal=True, seed=19)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    _verify("f16", o, q, COUNTS, ks, vs, dict(causal=True), slopes, "alibi/regime/" + route)
    # the steep head under causal: every weight but the newest key's is below exp(-50 + 16): o is that key's value row
    cu = _cu(COUNTS, "cpu").tolist()
    atol, rtol, _ = T.FWD_TOL["f16"]
    for b, n in enumerate(COUNTS):
        for i in range(n):
            v_new = _np(vs[b][6 // (H // HK), ks[b].shape[1] - n + i])
            got = _np(o[cu[b] + i, 6])
            assert (np.abs(got - v_new) <= atol + rtol * np.abs(v_new)).all(), (b, i)


# ---- 5. train / serve agreement ---------------------------------------------------------------------------------------------------------
def test_dense_call_with_attn_bias_and_cached_call_agree():
    dtype, D, n = "f16", 64, 150
    slopes = std_slopes(H)
    g = torch.Generator(device="cuda").manual_seed(23)
    q4, k4, v4 = (torch.randn(1, h, n, D, device="cuda", generator=g).to(DT[dtype]) for h in (H, HK, HK))
    bias = torch.from_numpy(alibi_matrix(slopes.numpy(), n, n)).to(device="cuda", dtype=DT[dtype])
    with torch.no_grad():
        o_dense = _F().flash_cosine_sim_attention(q4, k4, v4, attn_bias=bias, causal=True)
        kc, vc = torch.zeros(1, HK, 256, D, device="cuda", dtype=DT[dtype]), torch.zeros(1, HK, 256, D, device="cuda", dtype=DT[dtype])
        pk = lambda t: t[0].permute(1, 0, 2).contiguous()
        o_cache = _alibi(pk(q4), kc, vc, _cu([n]), pk(k4), pk(v4), _i32([0]), causal=True, alibi_slopes=slopes.cuda())
    ref = _reference(pk(q4), [n], [k4[0]], [v4[0]], dict(causal=True), slopes)
    import cases
    cond = cases.logit_cond(dtype, 8.0, 1, True)
    TK._check(dtype, o_cache, ref, "alibi/serve", cond)
    TK._check(dtype, o_dense[0].permute(1, 0, 2), ref, "alibi/train", cond)


# ---- 6. lse, and rows without a visible key ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", [("bf16", 128), ("f16", 64)])
def test_lse_includes_the_bias(dtype, D):
    import lse_reference as R
    import tolerances_lse as TL
    slopes = std_slopes(H)
    o, lse, q, ks, vs = _run(dtype, D, COUNTS, CACHED, CAP, slopes, MIXED, causal=True, seed=29)
    got = _np(lse)
    raw = _reference(q, COUNTS, ks, vs, dict(causal=True), slopes, with_lse=True)[1]
    assert np.isfinite(got).all() and np.isfinite(raw).all()
    d_raw = float(np.abs(got - raw).max())
    assert T.check(f"alibi/{dtype}/lse-raw", dtype, d_raw, R.derived_lse_bound(dtype, 8.0, 1, True)), d_raw
    ops = _reference(q, COUNTS, ks, vs, dict(causal=True), slopes, operand_dtype=dtype, with_lse=True)[1]
    d_ops = float(np.abs(got - ops).max())
    assert T.check(f"alibi/{dtype}/lse-operands", dtype, d_ops, TL.LSE_TOL[dtype]), d_ops


def test_rows_without_a_visible_key():
    """no append and nothing cached, or N_b > L_b under causal: o = 0, lse = -inf"""
    counts, cached = [3, 5, 20], [0, 2, 100]
    q, kc, vc, _, _ = TR._inputs("bf16", H, HK, 128, counts, 128, 31, append=False)
    for chunk_rows in (ALL_DECODE, ALL_CHUNK):
        with torch.no_grad():
            o, lse = _alibi(q, kc, vc, _cu(counts), None, None, _i32(cached), return_lse=True, causal=True, chunk_rows=chunk_rows,
                            alibi_slopes=std_slopes(H).cuda())
        assert (o[:3] == 0).all() and torch.isneginf(lse[:3]).all()            # L = 0
        assert (o[3:6] == 0).all() and torch.isneginf(lse[3:6]).all()          # rows 0 .. 2 of N = 5 over L = 2
        assert torch.isfinite(lse[6:]).all() and torch.isfinite(o).all()


# ---- 7. the call stays inside its buffers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype,D,heads,hk,page,fp8,window,per_seq", [("fp8_paged", "bf16", 128, 8, 2, 16, True, None, True),
                                                                           ("window", "f16", 64, 5, 1, 0, False, (70, 3), False)])
def test_alibi_call_stays_inside_its_buffers(name, dtype, D, heads, hk, page, fp8, window, per_seq):
    """test_gpu_kvcache_step.test_step_call_stays_inside_its_buffers for fcsa_forward_kvcache_alibi: q, k_new, v_new, the caches, the scales,
    the tables AND the slopes ([B, H] in one case, [H] in the other) inside one arena pre-filled with 0xFF bytes with guard bands between
    them; o and lse are strided views of larger buffers; the workspace has exactly the size the query gives.  No guard byte changes, what
    the call does not own keeps its fill, every owned element is written (0xFF.. is NaN in every type here), and the result is the Python
    call's.  chunk_rows = 128 routes the 130-token sequence (and at G = 4 / 5 the 37-token one) to the chunk kernel, the rest to the decode
    kernel, so both new entry points run; G * N_b is no multiple of 16 or 128, so both have rows past a tile's end."""
    from flash_cosine_sim_attention_amd import _lib
    from test_gpu_buffer_bounds import Arena, FILL
    lib = _lib.load()
    dt = DT[dtype]
    counts, cached, cap = [1, 0, 37, 130, 3], [5, 40, 0, 100, 200], 256
    B, total = len(counts), sum(counts)
    mb = cap // page if page else 0
    nb = B * mb + 2
    ces = 1 if fp8 else 2
    cache_elems = (nb * page if page else B * cap) * hk * D
    prob = _lib.problem(dt, (B, heads, hk, max(counts), cap, D), True, False, True, 1, 8.0)
    kv = _lib.KvCache()
    kv.capacity, kv.page_size, kv.num_blocks, kv.new_len = cap, page, nb if page else 0, 1
    seqs = _lib.Varlen(None, None, total, 0)
    st = _lib.KvCacheStep(128, 0, -1, 0, 0)
    win = _lib.Window(*window) if window else None
    winp = C.byref(win) if window else None
    wsb = int(lib.fcsa_forward_kvcache_step_workspace_bytes(C.byref(prob), C.byref(kv), C.byref(seqs), None, winp, C.byref(st)))
    assert wsb >= total * heads * (D + 2) * 4
    ar = Arena((total + 5) * heads * (D + 8) * 2 + (total + 5) * (heads + 3) * 4 + (total * heads * D + 2 * total * hk * D) * 2
               + 2 * cache_elems * ces + 4 * (2 * B + 1 + B * max(mb, 1)) + 8 * B * hk + 4 * B * heads + wsb + 44 * (4096 + 256))
    g = torch.Generator(device="cuda").manual_seed(D)

    def rnd(shape):
        t = ar.take(shape, dt)
        t.copy_(torch.randn(shape, device="cuda", dtype=torch.float32, generator=g).to(dt))
        return t

    q, kn, vn = rnd((total, heads, D)), rnd((total, hk, D)), rnd((total, hk, D))
    cshape = (nb, hk, page, D) if page else (B, hk, cap, D)
    quant = {}
    if fp8:
        kc, vc = ar.take(cshape, torch.uint8), ar.take(cshape, torch.uint8)
        kc.copy_(torch.randint(0, 0x78, cshape, device="cuda", generator=g, dtype=torch.uint8))      # finite positive codes
        vc.copy_(torch.randint(0, 0x78, cshape, device="cuda", generator=g, dtype=torch.uint8))
        ks, vs = ar.take((B, hk), torch.float32), ar.take((B, hk), torch.float32)
        ks.copy_(torch.rand(B, hk, device="cuda", generator=g) + 0.5), vs.copy_(torch.rand(B, hk, device="cuda", generator=g) + 0.5)
        quant = dict(k_scale=ks, v_scale=vs)
    else:
        kc, vc = rnd(cshape), rnd(cshape)
    slopes = ar.take((B, heads) if per_seq else (heads,), torch.float32)
    slopes.copy_((std_slopes(heads)[None] * (1 + torch.arange(B, dtype=torch.float32)[:, None] / 4) if per_seq else std_slopes(heads)).cuda())
    cu, sl = ar.take((B + 1,), torch.int32), ar.take((B,), torch.int32)
    cu.copy_(_cu(counts)), sl.copy_(_i32(cached))
    table = None
    if page:
        table = ar.take((B, mb), torch.int32)
        table.copy_(torch.randperm(nb, generator=torch.Generator().manual_seed(1))[:B * mb].reshape(B, mb).to(torch.int32))
    o_full, lse_full = ar.take((total + 5, heads, D + 8), dt), ar.take((total + 5, heads + 3), torch.float32)
    o, lse = o_full[2:2 + total, :, :D], lse_full[3:3 + total, 1:1 + heads]
    ws = ar.take((wsb,), torch.uint8)
    assert ws.data_ptr() % 256 == 0
    inputs = [q, kn, vn, cu, sl, slopes] + ([table] if page else []) + list(quant.values())
    before = [t.clone() for t in inputs]
    k_ref, v_ref = kc.clone(), vc.clone()

    packed = lambda t: _lib.Tensor(t.data_ptr(), 0, t.stride(1), t.stride(0))
    kv.k_cache, kv.v_cache = _lib.tensor4(kc), _lib.tensor4(vc)
    kv.k_new, kv.v_new = packed(kn), packed(vn)
    kv.cache_seqlens = sl.data_ptr()
    if page:
        kv.block_table, kv.block_table_stride = table.data_ptr(), mb
    seqs = _lib.Varlen(cu.data_ptr(), None, total, 0)
    none = _lib.Tensor(None, 0, 0, 0)
    fa = _lib.ForwardArgs(prob, packed(q), none, none, packed(o), None, None, None, _lib.NormState(None, None, None, None), ws.data_ptr(), wsb,
                          torch.cuda.current_stream().cuda_stream)
    lo = _lib.LseOut(lse.data_ptr(), 0, lse.stride(1), lse.stride(0))
    al = _lib.Alibi(slopes.data_ptr(), heads if per_seq else 0, 1, 0)
    qz = None
    if fp8:
        qz = _lib.KvCacheQuant()
        qz.cache_dtype, qz.k_scale, qz.v_scale = _lib.FCSA_CACHE_E4M3, ks.data_ptr(), vs.data_ptr()
        qz.k_scale_stride0, qz.k_scale_stride1, qz.v_scale_stride0, qz.v_scale_stride1 = hk, 1, hk, 1
    _lib.check(lib.fcsa_forward_kvcache_alibi(C.byref(fa), C.byref(kv), C.byref(seqs), C.byref(qz) if fp8 else None, winp, C.byref(st),
                                              C.byref(al), C.byref(lo)), "fcsa_forward_kvcache_alibi")
    torch.cuda.synchronize()
    assert ar.guards_intact(), "a byte outside the call's buffers was written"
    for t, b in zip(inputs, before):
        assert torch.equal(t, b), "an input changed"
    assert torch.isfinite(o).all() and not torch.isnan(lse).any()
    own = torch.zeros_like(o_full, dtype=torch.bool)
    own[2:2 + total, :, :D] = True
    assert (o_full.view(torch.int16)[~own] == -1).all(), "an element of the o buffer outside the view was written"
    own = torch.zeros_like(lse_full, dtype=torch.bool)
    own[3:3 + total, 1:1 + heads] = True
    assert (lse_full.view(torch.int32)[~own] == -1).all(), "an element of the lse buffer outside the view was written"
    typed = (lambda t: t.view(E4M3)) if fp8 else (lambda t: t)
    with torch.no_grad():
        o_py, lse_py = _alibi(q, typed(k_ref), typed(v_ref), cu, kn, vn, sl, block_table=table, max_seqlen_q=max(counts), causal=True,
                              return_lse=True, chunk_rows=128, window_size=window or (-1, -1), alibi_slopes=slopes, **quant)
    torch.cuda.synchronize()
    assert torch.equal(_bits(o), _bits(o_py)) and torch.equal(_bits(lse), _bits(lse_py))
    assert torch.equal(_bits(kc), _bits(k_ref)) and torch.equal(_bits(vc), _bits(v_ref))
    assert FILL == 0xFF


# ---- 8. graph capture with device tables and device slopes ------------------------------------------------------------------------------
def test_graph_capture_and_replay_with_changed_slopes_and_lengths():
    dtype, D = "bf16", 128
    q, kc, vc, kn, vn = TR._inputs(dtype, H, HK, D, COUNTS, CAP, 37)
    cu, sl, slopes = _cu(COUNTS), _i32(CACHED), std_slopes(H).cuda()
    kw = dict(max_seqlen_q=max(COUNTS), max_seqlen_k=CAP, return_lse=True, causal=True, chunk_rows=MIXED, max_decode_tokens=sum(COUNTS))
    k1, v1 = kc.clone(), vc.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream), torch.no_grad():
        _alibi(q, k1, v1, cu, kn, vn, sl, alibi_slopes=slopes, **kw)          # warm up: allocator and module loading
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        o_g, lse_g = _alibi(q, k1, v1, cu, kn, vn, sl, alibi_slopes=slopes, **kw)
    cached2 = [c // 2 for c in CACHED]
    sl.copy_(_i32(cached2))
    slopes.mul_(3.0)
    graph.replay()
    torch.cuda.synchronize()
    k2, v2 = kc.clone(), vc.clone()
    with torch.no_grad():
        o_e, lse_e = _alibi(q, k2, v2, cu, kn, vn, _i32(cached2), alibi_slopes=(std_slopes(H) * 3.0).cuda(), **kw)
    assert torch.equal(_bits(o_g), _bits(o_e)) and torch.equal(_bits(lse_g), _bits(lse_e))


# ---- 9. the C entry, called directly ----------------------------------------------------------------------------------------------------
def test_c_entry_directly():
    from flash_cosine_sim_attention_amd import _lib
    lib = _lib.load()
    dtype, D, counts, cached, cap = "f16", 64, [3, 20], [100, 7], 256
    q, kc, vc, kn, vn = TR._inputs(dtype, H, HK, D, counts, cap, 41)
    total = sum(counts)
    o = torch.full_like(q, float("nan"))
    lse = torch.full((total, H), float("nan"), device="cuda")
    cu, sl, slopes = _cu(counts), _i32(cached), std_slopes(H).cuda()
    args = _lib.ForwardArgs()
    args.p = _lib.problem(DT[dtype], (len(counts), H, HK, max(counts), cap, D), True, False, True, 1, 8.0)
    tens = lambda t: _lib.Tensor(t.data_ptr(), 0, t.stride(1), t.stride(0))
    args.q, args.o = tens(q), tens(o)
    kv = _lib.KvCache()
    kv.k_cache = _lib.Tensor(kc.data_ptr(), kc.stride(0), kc.stride(1), kc.stride(2))
    kv.v_cache = _lib.Tensor(vc.data_ptr(), vc.stride(0), vc.stride(1), vc.stride(2))
    kv.k_new, kv.v_new = tens(kn), tens(vn)
    kv.cache_seqlens, kv.capacity, kv.new_len = sl.data_ptr(), cap, 1
    seqs = _lib.Varlen(cu.data_ptr(), None, total, 0)
    st = _lib.KvCacheStep(16, 0, -1, 0, 0)
    need = int(lib.fcsa_forward_kvcache_step_workspace_bytes(C.byref(args.p), C.byref(kv), C.byref(seqs), None, None, C.byref(st)))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
    args.workspace, args.workspace_bytes = ws.data_ptr(), need
    args.stream = torch.cuda.current_stream().cuda_stream
    lo = _lib.LseOut(lse.data_ptr(), 0, lse.stride(1), lse.stride(0))
    al = _lib.Alibi(slopes.data_ptr(), 0, 1, 0)
    k0 = kc.clone()
    bad = _lib.Alibi(slopes.data_ptr(), 0, 1, 7)
    assert lib.fcsa_forward_kvcache_alibi(C.byref(args), C.byref(kv), C.byref(seqs), None, None, C.byref(st), C.byref(bad), C.byref(lo)) == -1
    assert lib.fcsa_forward_kvcache_alibi(C.byref(args), C.byref(kv), C.byref(seqs), None, None, C.byref(st), None, C.byref(lo)) == -1
    assert need > 0
    args.workspace_bytes = need - 1                                         # FCSA_ERR_WORKSPACE: the step call's workspace rule
    assert lib.fcsa_forward_kvcache_alibi(C.byref(args), C.byref(kv), C.byref(seqs), None, None, C.byref(st), C.byref(al), C.byref(lo)) == -4
    args.workspace_bytes = need
    torch.cuda.synchronize()
    assert torch.equal(_bits(kc), _bits(k0)) and torch.isnan(o).all()      # refused before any launch
    rc = lib.fcsa_forward_kvcache_alibi(C.byref(args), C.byref(kv), C.byref(seqs), None, None, C.byref(st), C.byref(al), C.byref(lo))
    assert rc == 0, _lib.last_error() if hasattr(_lib, "last_error") else rc
    torch.cuda.synchronize()
    k2, v2 = k0.clone(), vc.clone()
    v2[:] = TR._inputs(dtype, H, HK, D, counts, cap, 41)[2]
    with torch.no_grad():
        o_e, lse_e = _alibi(q, k2, v2, cu, kn, vn, sl, max_seqlen_q=max(counts), max_seqlen_k=cap, return_lse=True, causal=True, chunk_rows=16,
                            alibi_slopes=slopes)
    assert torch.equal(_bits(o), _bits(o_e)) and torch.equal(_bits(lse), _bits(lse_e)) and torch.equal(_bits(kc), _bits(k2))


# ---- 10. zero sizes ---------------------------------------------------------------------------------------------------------------------
def test_zero_sizes():
    dt = torch.bfloat16
    slopes = std_slopes(H).cuda()
    kc, vc = torch.zeros(2, HK, 64, 128, device="cuda", dtype=dt), torch.zeros(2, HK, 64, 128, device="cuda", dtype=dt)
    q = torch.zeros(0, H, 128, device="cuda", dtype=dt)
    o, lse = _alibi(q, kc, vc, _cu([0, 0]), None, None, _i32([5, 0]), return_lse=True, alibi_slopes=slopes)
    assert o.shape == (0, H, 128) and lse.shape == (0, H)
    q = torch.randn(4, H, 128, device="cuda").to(dt)
    o, lse = _alibi(q, kc, vc, _cu([4, 0]), None, None, _i32([0, 0]), return_lse=True, alibi_slopes=slopes)      # nothing cached
    assert (o == 0).all() and torch.isneginf(lse).all()
