"""Decoding against MXFP4 caches on the GPU (flash_cosine_sim_attention_mxfp4_with_kvcache, fcsa_forward_kvcache_mx).

The reference is the float64 oracle on the DEQUANTISED caches as the call left them (so the append is part of it), under
test_gpu_kvcache.py::_verify with its bars (tolerances.FWD_TOL, cases.logit_cond): every cache value is exact in f16 and bf16, so the
kernel owes the 16-bit kernel's accuracy and there is no tolerance of its own.  The append is compared byte for byte with mxfp4_quantize
on the CPU."""
import numpy as np
import pytest
import torch

import lse_reference as LR
import test_gpu_kvcache as TK
import tolerances_lse as TL

pytestmark = pytest.mark.gpu

DT = TK.DT


def _F():
    import flash_cosine_sim_attention_amd as F
    return F


def _rnd(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32)


def _caches(rnd, *shape):
    """(k codes, v codes, k scales, v scales) of random caches [*shape] (the last entry: D), in the function's order"""
    (kc, ks), (vc, vs) = _F().mxfp4_quantize(rnd(*shape)), _F().mxfp4_quantize(rnd(*shape))
    return kc, vc, ks, vs


def _dense(mx, dt):
    kc, vc, ks, vs = mx
    return _F().mxfp4_dequantize(kc, ks, dt), _F().mxfp4_dequantize(vc, vs, dt)


GRID = [(f"{dtype}_d{D}_n{N}", dtype, D, N, i % 2 == 0, (8, 2, 1)[i % 3])
        for i, (dtype, D, N) in enumerate((dt, d, n) for dt in ("bf16", "f16") for d in (32, 64, 96, 128) for n in (1, 3, 16))]


@pytest.mark.parametrize("name,dtype,D,N,causal,Hk", GRID, ids=[c[0] for c in GRID])
def test_mxfp4_grid(name, dtype, D, N, causal, Hk):
    H, B, cap, dt = 8, 3, 300, DT[dtype]
    n_new = (0, 1, N)[D % 3]
    rnd = _rnd(sum(map(ord, name)))
    q, mx = rnd(B, H, N, D).to(dt), _caches(rnd, B, Hk, cap, D)
    kn, vn = (rnd(B, Hk, n_new, D).to(dt), rnd(B, Hk, n_new, D).to(dt)) if n_new else (None, None)
    seq = [0, 17, cap - n_new] if N == 1 else [5, 130, cap - n_new]      # empty (N = 1, no append), one partial block, a full cache
    lens = [s + n_new for s in seq]
    o = _F().flash_cosine_sim_attention_mxfp4_with_kvcache(q, *mx, k_new=kn, v_new=vn, cache_seqlens=torch.tensor(seq, dtype=torch.int32, device="cuda"),
                                                           causal=causal)
    ks, vs = TK._seqs(*_dense(mx, dt), lens)
    TK._verify(dtype, o, q, ks, vs, dict(causal=causal), "mxfp4/" + name)
    for b, L in enumerate(lens):
        if L == 0:
            assert (o[b] == 0).all(), (name, b)


# l2norm groups, one row per path of the kernel's reduction (quarters of Q = D / 4 features per lane): the sum crosses a lane pair (two
# quarters per group), stays in the lane (whole groups inside a quarter), or -- D = 96 with 32 or 16 features -- straddles the quarters
GROUPS = [("bf16", 128, 2, 8.0), ("bf16", 128, 4, 2.0), ("f16", 128, 16, 1.0), ("bf16", 64, 8, 1.0), ("bf16", 64, 2, 4.0), ("f16", 32, 4, 2.0),
          ("bf16", 96, 2, 8.0), ("f16", 96, 3, 2.0), ("bf16", 96, 6, 2.0), ("bf16", 96, 4, 2.0), ("f16", 96, 12, 1.0)]      # f16, scale x groups > 11: per-row shift


@pytest.mark.parametrize("dtype,D,groups,scale", GROUPS, ids=[f"{c[0]}_d{c[1]}_groups{c[2]}" for c in GROUPS])
def test_mxfp4_groups(dtype, D, groups, scale):
    B, H, Hk, N, cap, dt, lens = 2, 8, 2, 3, 96, DT[dtype], [96, 41]
    rnd = _rnd(D + groups)
    q, mx = rnd(B, H, N, D).to(dt), _caches(rnd, B, Hk, cap, D)
    kw = dict(groups=groups, scale=scale, causal=groups % 2 == 0)
    o = _F().flash_cosine_sim_attention_mxfp4_with_kvcache(q, *mx, cache_seqlens=torch.tensor(lens, dtype=torch.int32, device="cuda"), **kw)
    ks, vs = TK._seqs(*_dense(mx, dt), lens)
    TK._verify(dtype, o, q, ks, vs, kw, f"mxfp4/groups_{dtype}_d{D}_{groups}")


def _every_code(rows, D, step):
    """codes [rows, D / 2] running through all 256 byte values -- every nibble value in both positions -- and scale bytes [rows, D / 32]
    running through 112 ... 140: the range the library reads, one below and one above (read as 113 and 139)"""
    codes = (torch.arange(rows * D // 2, dtype=torch.int64) * step % 256).to(torch.uint8).view(rows, D // 2)
    scales = (112 + torch.arange(rows * D // 32, dtype=torch.int64) * 5 % 29).to(torch.uint8).view(rows, D // 32)
    return codes, scales


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("l2norm", [True, False], ids=["l2norm", "raw"])
def test_mxfp4_every_code_and_scale(dtype, l2norm):
    """K: every code under every scale, position by position.  V: every code, with one scale byte per (K/V head, feature block) -- the
    outputs of a block are then that power of two times outputs of unit size, and o and the reference are compared divided by it (exact),
    which is where the bars of _verify apply.  Without l2norm_qk q and scale are powers of two down, so that the logits are of order 1."""
    B, H, Hk, N, D, cap, dt = 2, 4, 2, 3, 128, 96, DT[dtype]
    kc, ks = (t.view(B, Hk, cap, -1).cuda() for t in _every_code(B * Hk * cap, D, 37))
    vc = _every_code(B * Hk * cap, D, 91)[0].view(B, Hk, cap, -1).cuda()
    col = torch.tensor([[112, 119, 131, 140], [127, 139, 113, 124]], dtype=torch.uint8, device="cuda")      # [Hk, D / 32]
    vs = col.view(1, Hk, 1, D // 32).expand(B, Hk, cap, D // 32).contiguous()
    q = _rnd(7)(B, H, N, D) * (1.0 if l2norm else 2.0 ** -8)
    kw = dict(causal=True) if l2norm else dict(causal=False, l2norm_qk=False, scale=2.0 ** -9)
    o = _F().flash_cosine_sim_attention_mxfp4_with_kvcache(q.to(dt), kc, vc, ks, vs, cache_seqlens=torch.tensor([cap, 77], dtype=torch.int32, device="cuda"), **kw)
    unit = torch.exp2(col.clamp(113, 139).float() - 127).repeat_interleave(32, dim=1)      # [Hk, D]
    kd, vd = _F().mxfp4_dequantize(kc, ks, torch.float64), _F().mxfp4_dequantize(vc, vs, torch.float64) / unit.double().view(1, Hk, 1, D)
    kseq, vseq = TK._seqs(kd, vd, [cap, 77])
    o_unit = o.float() / unit.repeat_interleave(H // Hk, dim=0).view(1, H, 1, D)
    TK._verify(dtype, o_unit, q.to(dt), kseq, vseq, kw, f"mxfp4/every_code_{dtype}_{l2norm}")


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_mxfp4_one_key_returns_the_value_row(dtype):
    """One visible key in the per-row-shift regime: P~ = 1 and l = 1, so o is the dequantised V row exactly -- every code under every scale
    byte 112 ... 140, whatever the position of the block."""
    B, H, D, dt = 58, 2, 128, DT[dtype]
    vc, vs = (t.view(B, H, 1, -1).repeat(1, 1, 16, 1).cuda() for t in _every_code(B * H, D, 53))
    kc, _, ks, _ = _caches(_rnd(3), B, H, 16, D)
    q = _rnd(4)(B, H, 1, D).to(dt)
    o = _F().flash_cosine_sim_attention_mxfp4_with_kvcache(q, kc, vc, ks, vs, cache_seqlens=torch.ones(B, dtype=torch.int32, device="cuda"), scale=120)
    assert torch.equal(o, _F().mxfp4_dequantize(vc, vs, dt)[:, :, :1])


def _append_rows(B, Hk, n, D, dt):
    """new rows whose blocks hold exact ties (2.5, 5 and 0.25 times a power of two), values beyond 6 * 2^12, an all-zero block and blocks
    whose amax is a power of two, among blocks of random values of many sizes (all finite in f16)"""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, Hk, n, D, generator=g) * torch.exp2(torch.randint(-18, 14, (B, Hk, n, D // 32, 1), generator=g).float()).expand(-1, -1, -1, -1, 32).flatten(-2)
    ties = torch.tensor([2.5, 5.0, 0.25, 0.75, 1.25, 1.75, 3.5, 6.0, -2.5, -5.0, -0.25, 7.0, 4.0, 3.0, 1.0, -6.5] * 2)
    x[0, 0, 0, :32] = ties                    # amax 7: the grid itself
    x[0, 0, 1, :32] = ties * 2.0 ** -9
    x[0, 1, 0, 32:64] = ties * 2.0 ** 6
    x[1, 0, 0, :32] = 0.0
    x[1, 0, 1, :32] = torch.tensor([4.0, -1.0, 0.5, 0.0] * 8)            # amax on a power of two
    x[1, 1, 0, :32] = torch.tensor([2.0 ** -13, 2.0 ** -15, 0.0, -2.0 ** -14] * 8)      # below the smallest scale
    x[1, 1, 1, 32:64] = torch.tensor([30000.0, -50000.0, 24576.0, 12288.0] * 8)         # beyond 6 * 2^12
    return x.to(dt)


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("D,ragged", [(64, False), (64, True), (96, True), (128, False), (128, True)])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_mxfp4_append_bytes(dtype, D, ragged, paged):
    """equal N: three new rows per sequence; ragged: the same six packed rows as two and four"""
    F, (B, Hk, H, n, cap, page), dt = _F(), (2, 2, 4, 3, 48, 16), DT[dtype]
    kn, vn = _append_rows(B, Hk, n, D, dt), _append_rows(B, Hk, n, D, dt).flip(2).neg()
    pack = lambda t: t.transpose(1, 2).flatten(0, 1)
    cu, seq, table = ([0, 2, 6], [14, 44], [[4, 1, 5], [0, 3, 2]]) if ragged else ([0, 3, 6], [14, 45], [[4, 1, 5], [0, 3, 2]])
    g = torch.Generator().manual_seed(5)
    lead = (6, Hk, page) if paged else (B, Hk, cap)
    before = [torch.randint(0, 256, (*lead, w), generator=g, dtype=torch.uint8) for w in (D // 2, D // 32, D // 2, D // 32)]      # kc, ks, vc, vs
    after = [t.cuda() for t in before]
    q = torch.randn(B, H, n, D, generator=g).to(dt).cuda()
    shaped = (lambda t: pack(t).cuda()) if ragged else (lambda t: t.cuda())
    F.flash_cosine_sim_attention_mxfp4_with_kvcache(shaped(q), after[0], after[2], after[1], after[3], k_new=shaped(kn), v_new=shaped(vn),
                                                    cu_seqlens_q=torch.tensor(cu, dtype=torch.int32) if ragged else None,
                                                    cache_seqlens=torch.tensor(seq, dtype=torch.int32), causal=True,
                                                    block_table=torch.tensor(table, dtype=torch.int32) if paged else None)
    want = [t.clone() for t in before]
    for new, (codes, scales) in ((kn, want[:2]), (vn, want[2:])):
        qc, qs = F.mxfp4_quantize(pack(new))
        for b in range(B):
            for i in range(cu[b + 1] - cu[b]):
                pos = seq[b] + i
                blk, off = (table[b][pos // page], pos % page) if paged else (b, pos)
                codes[blk, :, off], scales[blk, :, off] = qc[cu[b] + i], qs[cu[b] + i]
    for name, got, exp in zip(("k codes", "k scales", "v codes", "v scales"), after, want):
        assert torch.equal(got.cpu(), exp), (name, (got.cpu() != exp).nonzero()[:8].tolist())


def _lse_check(dtype, lse, q, kseq, kw, label):
    """lse [rows..., H] of every sequence against float64 on the operands the kernel is fed (tolerances_lse.LSE_TOL)"""
    for b, k in enumerate(kseq):
        if q[b].shape[1]:
            ref = LR.lse_rows(TK._np(q[b]), TK._np(k), operand_dtype=dtype, **kw)
            got = TK._np(lse[b])
            assert np.array_equal(np.isinf(ref), np.isinf(got)), (label, b)
            assert np.abs(np.where(np.isinf(ref), 0.0, got - ref)).max(initial=0.0) <= TL.LSE_TOL[dtype], (label, b)


COMBOS = ["ragged_lse", "window", "splits", "strided_pool", "graph"]


@pytest.mark.parametrize("combo", COMBOS)
def test_mxfp4_combinations(combo):
    """ragged cu_seqlens_q with N_b = 0 and the lse; a window (one query per sequence: its visible keys are a slice); many key splits on a
    2k-key cache; a strided paged pool; device tables inside a captured graph, replayed once"""
    F, dtype, dt, D, H, Hk = _F(), "bf16", torch.bfloat16, 128, 8, 2
    api, rnd, dev = F.flash_cosine_sim_attention_mxfp4_with_kvcache, _rnd(len(combo)), "cuda"
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    if combo == "ragged_lse":
        counts, seq, cap = [3, 0, 1, 5], [40, 7, 0, 59], 64
        cu = np.concatenate([[0], np.cumsum(counts)]).tolist()
        q, mx = rnd(cu[-1], H, D).to(dt), _caches(rnd, len(counts), Hk, cap, D)
        o, lse = api(q, *mx, cu_seqlens_q=i32(cu), k_new=rnd(cu[-1], Hk, D).to(dt), v_new=rnd(cu[-1], Hk, D).to(dt), cache_seqlens=i32(seq), causal=True,
                     return_lse=True)
        kd, vd = _dense(mx, dt)
        for b, (n, s) in enumerate(zip(counts, seq)):
            if n:
                qb = q[cu[b]:cu[b + 1]].transpose(0, 1)[None]
                TK._verify(dtype, o[cu[b]:cu[b + 1]].transpose(0, 1)[None], qb, [kd[b, :, :s + n]], [vd[b, :, :s + n]], dict(causal=True), f"mxfp4/ragged{b}")
                _lse_check(dtype, [lse[cu[b]:cu[b + 1]].T], qb, [kd[b, :, :s + n]], dict(causal=True), f"mxfp4/ragged{b}")
        return
    if combo == "window":
        B, cap, left, seq = 3, 128, 40, [128, 41, 9]
        q, mx = rnd(B, H, 1, D).to(dt), _caches(rnd, B, Hk, cap, D)
        o = api(q, *mx, cache_seqlens=i32(seq), causal=True, window_size=(left, 0))
        kd, vd = _dense(mx, dt)
        TK._verify(dtype, o, q, [kd[b, :, max(L - 1 - left, 0):L] for b, L in enumerate(seq)], [vd[b, :, max(L - 1 - left, 0):L] for b, L in enumerate(seq)],
                   {}, "mxfp4/window")
        return
    if combo == "splits":
        q, mx = rnd(1, H, 2, D).to(dt), _caches(rnd, 1, Hk, 2048, D)
        o, lse = api(q, *mx, cache_seqlens=i32([2000]), causal=True, return_lse=True)
        kd, vd = _dense(mx, dt)
        TK._verify(dtype, o, q, [kd[0, :, :2000]], [vd[0, :, :2000]], dict(causal=True), "mxfp4/splits")
        _lse_check(dtype, lse, q, [kd[0, :, :2000]], dict(causal=True), "mxfp4/splits")
        return
    # a paged pool, [blocks, page, Hk, ...] in memory for "strided_pool"
    B, page, blocks, seq, table = 2, 16, 9, [70, 33], [[7, 2, 5, 0, 8], [3, 6, 1, 4, 4]]
    shape = (blocks, page, Hk, D) if combo == "strided_pool" else (blocks, Hk, page, D)
    mx = tuple(t.transpose(1, 2) if combo == "strided_pool" else t for t in _caches(rnd, *shape))
    q, kn, vn = rnd(B, H, 2, D).to(dt), rnd(B, Hk, 2, D).to(dt), rnd(B, Hk, 2, D).to(dt)
    run = lambda: api(q, *mx, k_new=kn, v_new=vn, cache_seqlens=i32(seq) if combo != "graph" else sl, block_table=i32(table) if combo != "graph" else tab,
                      max_seqlen_k=80)
    if combo == "graph":
        sl, tab = i32(seq), i32(table)
        eager = run()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            o = run()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o, eager)
    else:
        o = run()
    kd, vd = _dense(mx, dt)
    ks, vs = TK._seqs(kd, vd, [s + 2 for s in seq], torch.tensor(table))
    TK._verify(dtype, o, q, ks, vs, {}, "mxfp4/" + combo)
