"""Ragged decode steps on the GPU (flash_cosine_sim_attention_varlen_with_kvcache, fcsa_forward_kvcache_varlen): packed queries with a
per-sequence count against the key/value cache.

The contract: sequence b's rows are what flash_cosine_sim_attention_with_kvcache computes for that sequence alone.  Two references:
the float64 oracle per sequence under the policy and bars of test_gpu_kvcache.py (raw and operand-faithful passes, tolerances.FWD_TOL,
cases.logit_cond), and -- where both sides run one key split, so the arithmetic is the same instruction for instruction -- the existing
call itself, bit for bit, including the cache bytes after the append and NaN-filled guard regions."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_kvcache as TK
import test_gpu_kvcache_fp8 as T8
from test_gpu_buffer_bounds import Arena

pytestmark = pytest.mark.gpu

DT = TK.DT
E4M3 = torch.float8_e4m3fn

# the mixed batch: a first token into an empty cache, an empty sequence, a few speculative tokens, exactly one row tile (Hk == H), a ragged
# chunk into an empty cache, a plain decode deep in the cache, a prompt chunk of several row tiles
N_B = [1, 0, 5, 16, 37, 1, 130]
CACHED = [0, 17, 300, 5, 0, 1023, 200]
CAPACITY = 1200


def _api():
    import flash_cosine_sim_attention_amd as F
    return F.flash_cosine_sim_attention_varlen_with_kvcache


def _cu(counts, device="cuda"):
    c = [0]
    for n in counts:
        c.append(c[-1] + n)
    return torch.tensor(c, dtype=torch.int32, device=device)


def _i32(x, device="cuda"):
    return torch.tensor(x, dtype=torch.int32, device=device)


def _inputs(dtype, H, Hk, D, counts, cap, seed, append=True):
    """packed q [total, H, D], caches [B, Hk, cap, D], packed k_new / v_new [total, Hk, D]"""
    dt = DT[dtype]
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32).to(dt)
    B, total = len(counts), sum(counts)
    q = rnd(total, H, D)
    kc, vc = rnd(B, Hk, cap, D), rnd(B, Hk, cap, D)
    kn, vn = (rnd(total, Hk, D), rnd(total, Hk, D)) if append else (None, None)
    return q, kc, vc, kn, vn


def _paged(kc, vc, page, seed, spare=5):
    """The contiguous caches scattered over a NaN-filled pool in the vLLM [num_blocks, page, Hk, D] layout, passed transposed."""
    B, Hk, cap, D = kc.shape
    mb = cap // page
    nb = B * mb + spare
    table = torch.randperm(nb, generator=torch.Generator().manual_seed(seed))[:B * mb].reshape(B, mb).to(torch.int32)
    fill = 0x7f if kc.dtype == torch.uint8 else float("nan")
    pool_k = torch.full((nb, page, Hk, D), fill, device="cuda", dtype=kc.dtype)
    pool_v = torch.full_like(pool_k, fill)
    for b in range(B):
        for i in range(mb):
            pool_k[int(table[b, i])] = kc[b, :, i * page:(i + 1) * page].transpose(0, 1)
            pool_v[int(table[b, i])] = vc[b, :, i * page:(i + 1) * page].transpose(0, 1)
    return pool_k.transpose(1, 2), pool_v.transpose(1, 2), table


def _rows(t, cu, b):
    """sequence b's packed rows as [1, heads, N_b, D]"""
    return None if t is None else t[cu[b]:cu[b + 1]].permute(1, 0, 2).unsqueeze(0)


def _reference(q, counts, kseq, vseq, kw, operand_dtype=None):
    """The float64 oracle per sequence, packed like q: TK._reference on the batch-1 problem; under a window (kw["window_size"]) the same
    oracle call with the band as an additive bias, as test_gpu_window.py does for the equal-N call."""
    cu = _cu(counts, "cpu").tolist()
    out = np.zeros(q.shape)
    window = kw.get("window_size")
    for b, n in enumerate(counts):
        if n == 0 or kseq[b].shape[1] == 0:
            continue
        qb = _rows(q, cu, b)
        if window is None:
            o = TK._reference(qb, [kseq[b]], [vseq[b]], kw, operand_dtype)
        else:
            import cases
            from oracle import cosine_sim_oracle as O
            from test_gpu_window import band
            dtype = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}[q.dtype]
            scale, groups, l2, causal = kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True), kw.get("causal", False)
            dyn = cases.dynamic_shift_regime(dtype, scale, groups, l2, False)
            H, L = q.shape[1], kseq[b].shape[1]
            G = H // kseq[b].shape[0]
            kr, vr = (np.repeat(TK._np(x)[None], G, axis=1) for x in (kseq[b], vseq[b]))
            o = O.attention_forward_stats(TK._np(qb), kr, vr, scale=scale, groups=groups, causal=causal, l2norm_qk=l2,
                                          attn_bias=np.repeat(band(n, L, window[0], window[1], causal), H, axis=0),
                                          eps=1e-300 if dyn else 1e-10, operand_dtype=operand_dtype)[0]
        out[cu[b]:cu[b + 1]] = o[0].transpose(1, 0, 2)
    return out


def _verify(dtype, o, q, counts, kseq, vseq, kw, label, raw=True):
    """TK._verify's policy on packed rows: the raw pass with the bars scaled by cases.logit_cond, and (16-bit, l2norm) the
    operand-faithful pass with the fixed bars.  raw=False: the operand-faithful pass alone (16-bit, l2norm only; see
    test_ragged_many_splits_long_cache)."""
    import cases
    cond = cases.logit_cond(dtype, kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True))
    assert raw or (dtype != "f32" and kw.get("l2norm_qk", True))
    if raw:
        TK._check(dtype, o, _reference(q, counts, kseq, vseq, kw), label + "/raw", cond)
    if dtype != "f32" and kw.get("l2norm_qk", True):
        TK._check(dtype, o, _reference(q, counts, kseq, vseq, kw, operand_dtype=dtype), label + "/operands")


def _appended(kc, kn, counts, cached):
    """the contiguous cache after the append, computed with torch"""
    out = kc.clone()
    cu = _cu(counts, "cpu").tolist()
    for b, (s, n) in enumerate(zip(cached, counts)):
        out[b, :, s:s + n] = kn[cu[b]:cu[b + 1]].permute(1, 0, 2)
    return out


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


# ---- parity: the mixed batch over dtype x D x Hk x causal ---------------------------------------------------------------------------------

GRID = [(f"{dt}_d{d}_hk{hk}_{'causal' if c else 'full'}", dt, d, hk, c)
        for dt in ("bf16", "f16", "f32") for d in (16, 32, 64, 96, 128) for hk in (8, 2, 1) for c in (False, True)]


@pytest.mark.parametrize("name,dtype,D,Hk,causal", GRID, ids=[c[0] for c in GRID])
def test_ragged_parity_mixed_batch(name, dtype, D, Hk, causal):
    H = 8
    seed = sum(map(ord, name))
    q, kc, vc, kn, vn = _inputs(dtype, H, Hk, D, N_B, CAPACITY, seed)
    paged = seed % 2 == 1
    expect_k, expect_v = _appended(kc, kn, N_B, CACHED), _appended(vc, vn, N_B, CACHED)
    table = None
    if paged:
        kc, vc, table = _paged(kc, vc, 16, seed)
    with torch.no_grad():
        o = _api()(q, kc, vc, _cu(N_B), kn, vn, _i32(CACHED), block_table=None if table is None else table.cuda(), causal=causal)
    torch.cuda.synchronize()
    assert o.shape == q.shape and o.dtype == q.dtype
    lens = [s + n for s, n in zip(CACHED, N_B)]
    ks, vs = TK._seqs(kc, vc, lens, table)
    for b, L in enumerate(lens):                       # the append landed: every sequence's first L_b positions
        assert torch.equal(_bits(ks[b]), _bits(expect_k[b, :, :L])) and torch.equal(_bits(vs[b]), _bits(expect_v[b, :, :L])), (name, b)
    if not paged:
        assert torch.equal(_bits(kc), _bits(expect_k)) and torch.equal(_bits(vc), _bits(expect_v))
    _verify(dtype, o, q, N_B, ks, vs, dict(causal=causal), name)


RAGGED_N = [1, 5, 0, 21]          # + the regime's own N as the last sequence
RAGGED_CACHED = [600, 33, 100, 0, 7]


@pytest.mark.parametrize("name,dtype,D,N,H,Hk,kw", TK.REGIMES, ids=[c[0] for c in TK.REGIMES])
def test_ragged_regimes(name, dtype, D, N, H, Hk, kw):
    """The regime list of test_kvcache_regimes (exponent regimes, groups -- with the D = 96 widths of the LDS form --, l2norm off) on ragged
    query counts."""
    counts, cap = RAGGED_N + [N], 700
    l2 = kw.get("l2norm_qk", True)
    q, kc, vc, kn, vn = _inputs(dtype, H, Hk, D, counts, cap, seed=sum(map(ord, name)))
    q, kc = TK._unit_normalised(q, kc, kw.get("groups", 1), l2)
    _, kn = TK._unit_normalised(q, kn, 1, l2)
    with torch.no_grad():
        o = _api()(q, kc, vc, _cu(counts), kn, vn, _i32(RAGGED_CACHED), **kw)
    torch.cuda.synchronize()
    ks, vs = TK._seqs(kc, vc, [s + n for s, n in zip(RAGGED_CACHED, counts)])
    _verify(dtype, o, q, counts, ks, vs, kw, "ragged/" + name)


# ---- bit for bit against the existing call ---------------------------------------------------------------------------------------------

# one key split on both sides: max_seqlen_k = the capacity 240 < 2 * decode_min_split_keys(D) (>= 256 for every D <= 128)
BIT_N = [1, 0, 5, 16, 37, 1, 60]
BIT_CACHED = [0, 17, 150, 5, 0, 239, 100]
BIT_CAP = 240

BITWISE = [
    # id, dtype, D, H, Hk, fp8, kwargs
    ("bf16_d128_causal", "bf16", 128, 8, 2, False, dict(causal=True)),
    ("f16_d64_full", "f16", 64, 8, 8, False, dict()),
    ("f32_d32_causal", "f32", 32, 4, 1, False, dict(causal=True)),
    ("f32_d96_groups4_lds_form", "f32", 96, 4, 2, False, dict(groups=4, scale=4.0)),
    ("f16_d64_per_row_regime", "f16", 64, 8, 2, False, dict(scale=8.0, groups=2, causal=True)),
    ("bf16_d64_no_l2norm", "bf16", 64, 4, 2, False, dict(l2norm_qk=False, scale=1.0, causal=True)),
    ("bf16_d64_window_64_0", "bf16", 64, 8, 2, False, dict(window_size=(64, 0))),
    ("f16_d128_window_40_3", "f16", 128, 4, 4, False, dict(window_size=(40, 3))),
    ("f32_d16_window_causal", "f32", 16, 4, 2, False, dict(window_size=(20, -1), causal=True)),
    ("bf16_d96_groups2_window", "bf16", 96, 8, 2, False, dict(groups=2, window_size=(64, 0))),
    ("bf16_d128_fp8_causal", "bf16", 128, 8, 2, True, dict(causal=True)),
    ("f16_d64_fp8_window", "f16", 64, 8, 8, True, dict(window_size=(64, 0))),
    ("bf16_d96_fp8_groups4", "bf16", 96, 8, 2, True, dict(groups=4, scale=2.0)),
    ("f16_d32_fp8_no_l2norm", "f16", 32, 4, 1, True, dict(l2norm_qk=False, scale=1.0, causal=True)),
]


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("name,dtype,D,H,Hk,fp8,kw", BITWISE, ids=[c[0] for c in BITWISE])
def test_ragged_equals_per_sequence_call_bit_for_bit(name, dtype, D, H, Hk, fp8, kw, paged):
    """Each sequence's rows equal flash_cosine_sim_attention_with_kvcache on that sequence alone, bit for bit; the caches after the ragged
    append equal the caches after the per-sequence appends, byte for byte; positions beyond each sequence's length, the guard bands around
    the caches and the pages outside every table hold NaN before and after."""
    import flash_cosine_sim_attention_amd as F
    per_seq = F.flash_cosine_sim_attention_with_kvcache
    B, guard = len(BIT_N), 4096
    q, kc0, vc0, kn, vn = _inputs(dtype, H, Hk, D, BIT_N, BIT_CAP, seed=sum(map(ord, name)))
    if not kw.get("l2norm_qk", True):
        q, kc0 = TK._unit_normalised(q, kc0, 1, False)
        _, kn = TK._unit_normalised(q, kn, 1, False)
    quant = [{} for _ in range(B)]
    all_quant = {}
    if fp8:
        (kc0, ks), (vc0, vs) = T8._quantise(kc0), T8._quantise(vc0)
        kc0, vc0 = kc0.view(torch.uint8), vc0.view(torch.uint8)
        quant = [dict(k_scale=ks[b:b + 1], v_scale=vs[b:b + 1]) for b in range(B)]
        all_quant = dict(k_scale=ks, v_scale=vs)
    nan = 0x7f if fp8 else float("nan")                 # (0x7f: an e4m3fn NaN)
    for b, s in enumerate(BIT_CACHED):                   # slots beyond each sequence's length must never reach the output
        kc0[b, :, s:] = nan
        vc0[b, :, s:] = nan
    cu = _cu(BIT_N)
    cul = cu.tolist()
    sl = _i32(BIT_CACHED)
    typed = (lambda t: t.view(E4M3)) if fp8 else (lambda t: t)

    def caches():
        """two independent copies of the caches in their layout, with what must stay NaN around them"""
        if paged:
            pk, pv, table = _paged(kc0, vc0, 16, seed=len(name))
            return pk, pv, table.cuda(), [pk, pv]
        n = B * BIT_CAP * Hk * D
        arenas = [torch.full((2 * guard + n,), nan, device="cuda", dtype=kc0.dtype) for _ in range(2)]
        views = [a[guard:guard + n].view(B, BIT_CAP, Hk, D).transpose(1, 2) for a in arenas]
        views[0].copy_(kc0)
        views[1].copy_(vc0)
        return views[0], views[1], None, arenas

    ka, va, ta, hold_a = caches()
    kb, vb, tb, hold_b = caches()
    with torch.no_grad():
        o = _api()(q, typed(ka), typed(va), cu, kn, vn, sl, block_table=ta, **all_quant, **kw)
        ref = torch.zeros_like(q)
        for b in range(B):
            if BIT_N[b] == 0:
                continue
            if paged:
                ob = per_seq(_rows(q, cul, b), typed(kb), typed(vb), _rows(kn, cul, b), _rows(vn, cul, b), sl[b:b + 1], block_table=tb[b:b + 1],
                             **quant[b], **kw)
            else:
                ob = per_seq(_rows(q, cul, b), typed(kb[b:b + 1]), typed(vb[b:b + 1]), _rows(kn, cul, b), _rows(vn, cul, b), sl[b:b + 1],
                             **quant[b], **kw)
            ref[cul[b]:cul[b + 1]] = ob[0].permute(1, 0, 2)
    torch.cuda.synchronize()
    assert torch.isfinite(o.float()).all()
    assert torch.equal(_bits(o), _bits(ref)), f"{name}: {int((_bits(o) != _bits(ref)).sum())} elements differ"
    for x, y in zip(hold_a, hold_b):                    # whole arenas / pools: appended slots, untouched slots, guards, spare pages
        assert torch.equal(_bits(x), _bits(y)), name
    if not paged:
        for a in hold_a:
            isnan = (lambda t: t == 0x7f) if fp8 else torch.isnan
            assert isnan(a[:guard]).all() and isnan(a[-guard:]).all()
    # ... and the appended slots hold the new rows (fp8: their codes under the append rule)
    if not fp8 and not paged:
        assert torch.equal(_bits(ka), _bits(_appended(kc0, kn, BIT_N, BIT_CACHED)))
        assert torch.equal(_bits(va), _bits(_appended(vc0, vn, BIT_N, BIT_CACHED)))


# ---- many splits ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", [("bf16", 32), ("f16", 16), ("f32", 32), ("bf16", 128)])
def test_ragged_many_splits_long_cache(dtype, D):
    """A 32k cache on a small batch: tens of key splits, windows that end inside a 32-key block, ragged lengths and ragged counts; the
    combine reconciles every split of every packed row, in the static regime and (scale 16, groups 2) the per-row regime.
    float16 runs scale 16, groups 2 in the per-row-shift regime, and there it takes the operand-faithful comparison only, as the 16-bit
    per-row cases of test_gpu_window.py do: the two EXACT references are further apart than the raw bar before any kernel runs.  Float64 on
    random f16 inputs of this test's shapes (H 4, Hk 1, D 16, twelve seeds each; no kernel involved): raw against 16-bit operands differ
    elementwise (beyond rtol) by up to 6.95e-3 at N_b = 23, L_b = 576, 3.32e-3 at (4, 7779) and 2.85e-3 at (1, 32768) against the raw bar
    of 5.0e-3 (2.5e-3 x logit_cond 2), and by a rel-L2 of up to 1.26e-3, 2.19e-3 and 2.45e-3 against 1.7e-3 -- with 92 such rows in the
    batch the raw comparison cannot judge a kernel.  In the static regime (scale 8: at most 4.6e-4 against 2.5e-3) both passes run."""
    H, Hk, cap = 4, 1, 32768
    counts, cached = [1, 4, 23, 0], [cap - 1, 7775, 553, 9000]
    q, kc, vc, kn, vn = _inputs(dtype, H, Hk, D, counts, cap, seed=D + len(dtype))
    for kw in (dict(causal=True), dict(scale=16.0, groups=2)):
        kc_, vc_ = kc.clone(), vc.clone()
        with torch.no_grad():
            o = _api()(q, kc_, vc_, _cu(counts), kn, vn, _i32(cached), **kw)
        torch.cuda.synchronize()
        ks, vs = TK._seqs(kc_, vc_, [s + n for s, n in zip(cached, counts)])
        import cases
        per_row_16bit = dtype != "f32" and cases.dynamic_shift_regime(dtype, kw.get("scale", 8.0), kw.get("groups", 1), True, False)
        _verify(dtype, o, q, counts, ks, vs, kw, f"ragged_splits_{dtype}_d{D}_{sorted(kw)}", raw=not per_row_16bit)


# ---- bounds, table forms ----------------------------------------------------------------------------------------------------------------

def test_ragged_bounds_change_speed_not_result():
    """max_seqlen_q / max_seqlen_k at the true maxima, looser, left to their defaults and (a wrong bound) below the maxima: every call is
    within the parity bars (different bounds may choose different split counts, so the calls need not agree bit for bit)."""
    H, Hk, D, cap = 8, 2, 64, 8192
    counts, cached = [1, 3, 40, 1, 0, 9], [4000, 17, 2500, 8191, 100, 0]
    q, kc, vc, kn, vn = _inputs("bf16", H, Hk, D, counts, cap, seed=21)
    lens = [s + n for s, n in zip(cached, counts)]
    for bounds in (dict(max_seqlen_q=max(counts), max_seqlen_k=max(lens)), dict(max_seqlen_q=64, max_seqlen_k=6000 + max(lens) // 2),
                   dict(), dict(max_seqlen_q=10 ** 6, max_seqlen_k=10 ** 6), dict(max_seqlen_q=1, max_seqlen_k=64)):
        for kw in (dict(causal=True), dict(window_size=(300, 0)), dict(window_size=(100, 7))):
            kc_, vc_ = kc.clone(), vc.clone()
            with torch.no_grad():
                o = _api()(q, kc_, vc_, _cu(counts), kn, vn, _i32(cached), **bounds, **kw)
            torch.cuda.synchronize()
            ks, vs = TK._seqs(kc_, vc_, lens)
            _verify("bf16", o, q, counts, ks, vs, kw, f"ragged_bounds_{sorted(bounds.items())}_{sorted(kw)}")


def test_ragged_host_device_int_tables_agree():
    H, Hk, D, cap = 8, 8, 128, 1000
    counts = [1, 2, 0, 7, 1]
    q, kc, vc, kn, vn = _inputs("bf16", H, Hk, D, counts, cap, seed=5)
    cached = [0, 1, 500, 993, 999]
    run = lambda cu, sl, **kw: _api()(q, kc.clone(), vc.clone(), cu, kn, vn, sl, causal=True, **kw)
    with torch.no_grad():
        od = run(_cu(counts), _i32(cached))
        oh = run(_cu(counts, "cpu"), _i32(cached, "cpu"))
        om = run(_cu(counts, "cpu"), _i32(cached))
        # an int is the same length for every sequence; None (no append) is every sequence full
        oi = run(_cu(counts), 400)
        ot = run(_cu(counts), _i32([400] * len(counts)))
        of = _api()(q, kc, vc, _cu(counts), causal=True)
        oc = _api()(q, kc, vc, _cu(counts), cache_seqlens=cap, causal=True)
    torch.cuda.synchronize()
    assert torch.equal(od, oh) and torch.equal(od, om) and torch.equal(oi, ot) and torch.equal(of, oc)
    kc_, vc_ = kc.clone(), vc.clone()
    with torch.no_grad():
        o = _api()(q, kc_, vc_, _cu(counts), kn, vn, _i32(cached), causal=True)
    ks, vs = TK._seqs(kc_, vc_, [s + n for s, n in zip(cached, counts)])
    _verify("bf16", o, q, counts, ks, vs, dict(causal=True), "ragged_tables")
    assert torch.equal(o, od)


def test_ragged_rows_without_a_visible_key_are_zero():
    """No append: L_b = cache_seqlens[b]; under causal N_b > L_b leaves the first N_b - L_b rows without a key, L_b == 0 every row."""
    H, Hk, D, cap = 4, 2, 64, 128
    counts, cached = [3, 20, 40, 2], [0, 5, 40, 128]
    q, kc, vc, _, _ = _inputs("f16", H, Hk, D, counts, cap, seed=8, append=False)
    cu = _cu(counts).tolist()
    for kw in (dict(causal=True), dict(causal=True, scale=16.0, groups=2)):
        with torch.no_grad():
            o = _api()(q, kc, vc, _cu(counts), cache_seqlens=_i32(cached), **kw)
        torch.cuda.synchronize()
        assert (o[cu[0]:cu[1]] == 0).all()
        assert (o[cu[1]:cu[1] + 15] == 0).all() and torch.isfinite(o).all()
        ks, vs = TK._seqs(kc, vc, cached)
        _verify("f16", o, q, counts, ks, vs, kw, f"ragged_zero_rows_{sorted(kw)}")


def test_ragged_rejects_grad_and_bad_tables():
    q, kc, vc, kn, vn = _inputs("bf16", 2, 2, 32, [1, 2], 64, seed=1)
    with pytest.raises(RuntimeError):
        _api()(q.clone().requires_grad_(), kc, vc, _cu([1, 2]), cache_seqlens=3)
    with pytest.raises(ValueError):
        _api()(q, kc, vc, _cu([1, 3], "cpu"), kn, vn, _i32([1, 2]))
    with pytest.raises(ValueError):
        _api()(q, kc, vc, _cu([1, 2], "cpu"), kn, vn, _i32([1, 63], "cpu"))


# ---- binding: opcheck, graph capture ------------------------------------------------------------------------------------------------------

def test_ragged_opcheck():
    import flash_cosine_sim_attention_amd._torch_ops as ops
    fc = ops.load()
    counts = [2, 0, 5, 1]
    q, kc, vc, kn, vn = _inputs("bf16", 4, 2, 32, counts, 64, seed=2)
    cu, sl = _cu(counts), _i32([3, 40, 9, 63])
    op = fc.kvcache_varlen_forward.default
    torch.library.opcheck(op, (q, kc, vc, cu, kn, vn, sl, None, None, None, 5, 64, 8.0, True, True, 1, -1, -1))
    torch.library.opcheck(op, (q, kc, vc, cu, None, None, sl, None, None, None, 8, 64, 8.0, False, True, 2, 16, 0))
    pk, pv, table = _paged(kc, vc, 16, seed=3)
    torch.library.opcheck(op, (q, pk, pv, cu, kn, vn, sl, table.cuda(), None, None, 5, 64, 8.0, True, True, 1, -1, -1))
    (k8, ks), (v8, vs) = T8._quantise(kc), T8._quantise(vc)
    torch.library.opcheck(op, (q, k8.view(torch.uint8), v8.view(torch.uint8), cu, kn, vn, sl, None, ks, vs, 5, 64, 8.0, True, True, 1, -1, -1))


def test_ragged_graph_capture_and_replay():
    """One step with device tables, captured on a single stream (no parallel branches) and replayed with new queries, new rows, new lengths
    AND a new split of the packed rows among the sequences (total_q is the fixed shape; cu_seqlens_q is device data)."""
    H, Hk, D, cap, total = 8, 2, 64, 512, 12
    q, kc, vc, kn, vn = _inputs("bf16", H, Hk, D, [total, 0, 0], cap, seed=4)
    cu, sl = _i32([0, 1, 4, total]), _i32([10, 300, 77])
    f = _api()
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            f(q, kc, vc, cu, kn, vn, sl, max_seqlen_q=total, max_seqlen_k=cap, causal=True)      # warm-up (allocator, lazy init)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        kc_eager, vc_eager = kc.clone(), vc.clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = f(q, kc, vc, cu, kn, vn, sl, max_seqlen_q=total, max_seqlen_k=cap, causal=True)
        for step, (table, lens) in enumerate((([0, 1, 4, total], [11, 301, 78]), ([0, 6, 6, total], [12, 305, 80]), ([0, 2, 11, total], [400, 0, 90]))):
            q.copy_(torch.randn_like(q))
            kn.copy_(torch.randn_like(kn))
            vn.copy_(torch.randn_like(vn))
            cu.copy_(torch.tensor(table, dtype=torch.int32))
            sl.copy_(torch.tensor(lens, dtype=torch.int32))
            g.replay()
            ref = f(q, kc_eager, vc_eager, cu, kn, vn, sl, max_seqlen_q=total, max_seqlen_k=cap, causal=True)
            torch.cuda.synchronize()
            assert torch.equal(out, ref), step
            assert torch.equal(kc, kc_eager) and torch.equal(vc, vc_eager), step


# ---- buffer bounds through the C ABI ------------------------------------------------------------------------------------------------------

BOUNDS = [
    # id, dtype, D, H, Hk, counts, cached, capacity, page, fp8, window
    ("bf16_d128_mixed", "bf16", 128, 8, 2, [1, 0, 5, 16, 37, 1, 130], [0, 17, 300, 5, 0, 1023, 200], 1200, 0, False, None),
    ("f32_d96_paged", "f32", 96, 4, 4, [3, 1, 0, 19], [100, 0, 30, 620], 640, 32, False, None),
    ("f16_d64_fp8_window_paged", "f16", 64, 8, 1, [1, 7, 33, 2], [2000, 31, 1, 4094], 4096, 16, True, (100, 0)),
    ("bf16_d16_long_cache_splits", "bf16", 16, 2, 1, [2, 1, 9], [20000, 5, 19991], 20000 + 32, 0, False, None),
]


@pytest.mark.parametrize("name,dtype,D,H,Hk,counts,cached,cap,page,fp8,window", BOUNDS, ids=[c[0] for c in BOUNDS])
def test_ragged_call_stays_inside_its_buffers(name, dtype, D, H, Hk, counts, cached, cap, page, fp8, window):
    """q, o, k_new, v_new, the caches, the tables and a workspace of EXACTLY fcsa_forward_kvcache_varlen_workspace_bytes inside one arena
    pre-filled with 0xFF bytes (NaN in every float type), guard bands between them: no guard byte changes, the inputs keep their bits, no
    element of o is NaN (never written, or computed from workspace read before it was written)."""
    from flash_cosine_sim_attention_amd import _lib
    lib = _lib.load()
    dt = DT[dtype]
    es = torch.empty((), dtype=dt).element_size()
    ces = 1 if fp8 else es
    B, total = len(counts), sum(counts)
    mb = cap // page if page else 0
    nb = B * mb + 2
    prob = _lib.problem(dt, (B, H, Hk, max(counts), cap, D), True, False, True, 1, 8.0)
    cache_elems = (nb * page if page else B * cap) * Hk * D
    kv = _lib.KvCache()
    kv.capacity, kv.page_size, kv.num_blocks, kv.new_len = cap, page, nb if page else 0, 1
    seqs = _lib.Varlen(None, None, total, 0)
    win = _lib.Window(*window) if window else None
    qz = _lib.KvCacheQuant() if fp8 else None
    ref = lambda x: None if x is None else C.byref(x)
    ws_n = int(lib.fcsa_forward_kvcache_varlen_workspace_bytes(C.byref(prob), C.byref(kv), C.byref(seqs), ref(qz), ref(win)))
    assert ws_n > 0
    ar = Arena((2 * total * H * D + 2 * total * Hk * D) * es + 2 * cache_elems * ces + ws_n + 4 * (B + 1 + B * max(mb, 1) + 2 * B * Hk) + 30 * (4096 + 256))
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
    o = ar.take((total, H, D), dt)
    ws = ar.take((ws_n,), torch.uint8)
    inputs = [q, kn, vn, cu, sl]
    before = [t.clone() for t in inputs]
    packed = lambda t: _lib.Tensor(t.data_ptr(), 0, t.stride(1), t.stride(0))
    kv.k_cache, kv.v_cache = _lib.tensor4(kc), _lib.tensor4(vc)
    kv.k_new, kv.v_new = packed(kn), packed(vn)
    kv.cache_seqlens = sl.data_ptr()
    seqs.cu_seqlens_q = cu.data_ptr()
    none = _lib.Tensor(None, 0, 0, 0)
    fa = _lib.ForwardArgs(prob, packed(q), none, none, packed(o), None, None, None, _lib.NormState(None, None, None, None), ws.data_ptr(), ws_n,
                          torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.fcsa_forward_kvcache_varlen(C.byref(fa), C.byref(kv), C.byref(seqs), ref(qz), ref(win)), "fcsa_forward_kvcache_varlen")
    torch.cuda.synchronize()
    assert ar.guards_intact(), "a byte outside the call's buffers was written"
    for t, b in zip(inputs, before):
        assert torch.equal(t, b), "an input buffer was modified"
    bad = int((~torch.isfinite(o.float())).sum().item())
    assert bad == 0, f"o: {bad} element(s) are NaN -- never written, or computed from unwritten workspace"
    # one byte less of workspace is refused, nothing launched
    fa.workspace_bytes = ws_n - 1
    assert lib.fcsa_forward_kvcache_varlen(C.byref(fa), C.byref(kv), C.byref(seqs), ref(qz), ref(win)) == -4
