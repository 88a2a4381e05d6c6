"""Decoding against a key/value cache on the GPU (flash_cosine_sim_attention_with_kvcache, fcsa_forward_kvcache).

The contract: with L_b = cache_seqlens[b] + N_new, o[b] is what the dense op returns for q[b] against the first L_b cached positions of
sequence b after the append.  The reference is the float64 oracle run per sequence (K/V repeated over each query-head group); in the
per-row-shift regime the 16-bit cases are compared on the rounded operands, as in test_gpu_varlen.py.  The appended slots must hold
k_new / v_new bit for bit and every other slot of the cache must be untouched (NaN-filled guard regions)."""
import numpy as np
import pytest
import torch

import cases as C
import tolerances as T
from oracle import cosine_sim_oracle as O

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def _np(t):
    return t.detach().cpu().double().numpy()


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-3 * np.sqrt(max(b.size, 1))))


def _api():
    import flash_cosine_sim_attention_amd as F
    return F.flash_cosine_sim_attention_with_kvcache


def _reference(q, kseq, vseq, kw, operand_dtype=None):
    """o of every sequence: q [B, H, N, D] (torch), kseq / vseq lists of [Hk, L_b, D] (torch).  The row-sum clamp follows the library's
    regime (cases.dynamic_shift_regime: the per-row-shift regime normalises rows exactly, no 1e-10 clamp); operand_dtype: exact math on
    the 16-bit operands the S product is fed ("operand-faithful", as in test_gpu_parity.py)."""
    dtype = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}[q.dtype]
    scale, groups, l2norm = kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True)
    dyn = C.dynamic_shift_regime(dtype, scale, groups, l2norm, False)
    okw = dict(scale=scale, groups=groups, causal=kw.get("causal", False), l2norm_qk=l2norm, eps=1e-300 if dyn else 1e-10,
               operand_dtype=operand_dtype)
    B, H = q.shape[:2]
    out = np.zeros(q.shape)
    for b in range(B):
        L = kseq[b].shape[1]
        if L == 0:
            continue
        G = H // kseq[b].shape[0]
        ks, vs = (np.repeat(_np(x)[None], G, axis=1) for x in (kseq[b], vseq[b]))
        o, _ = O.attention_forward_stats(_np(q[b:b + 1]), ks, vs, **okw)
        out[b] = o[0]
    return out


def _check(dtype, o, ref, label, cond=1.0):
    atol, rtol, rel = T.FWD_TOL[dtype]
    go = _np(o)
    assert torch.isfinite(o).all(), label
    assert T.check(label + "/fwd-excess", dtype, float((np.abs(go - ref) - rtol * np.abs(ref)).max(initial=0.0)), atol * cond), label
    assert T.check(label + "/fwd-rel", dtype, _rel(go, ref), rel * cond), (label, _rel(go, ref), rel * cond)


def _verify(dtype, o, q, kseq, vseq, kw, label):
    """The parity test's policy: exact math on the raw inputs with the forward bars scaled by cases.logit_cond (the rounding of q^, k^ to
    16 bits is amplified by the logit range in any 16-bit evaluation), and -- 16-bit types -- exact math on the 16-bit operands with the
    fixed bars.  Without l2norm_qk the kernel feeds the raw 16-bit inputs and applies scale in float32, so the raw pass (cond 1) is
    already the operand-faithful one."""
    cond = C.logit_cond(dtype, kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True))
    _check(dtype, o, _reference(q, kseq, vseq, kw), label + "/raw", cond)
    if dtype != "f32" and kw.get("l2norm_qk", True):
        _check(dtype, o, _reference(q, kseq, vseq, kw, operand_dtype=dtype), label + "/operands")


def _seqs(k_cache, v_cache, lens, table=None):
    """Positions [0, L_b) of every sequence: lists of [Hk, L_b, D]."""
    ks, vs = [], []
    for b, L in enumerate(lens):
        if table is None:
            ks.append(k_cache[b, :, :L])
            vs.append(v_cache[b, :, :L])
        else:
            page = k_cache.shape[2]
            blocks = [int(x) for x in table[b, :(L + page - 1) // page].tolist()]
            kk = torch.cat([k_cache[i] for i in blocks], dim=1)[:, :L] if blocks else k_cache[0, :, :0]
            vv = torch.cat([v_cache[i] for i in blocks], dim=1)[:, :L] if blocks else v_cache[0, :, :0]
            ks.append(kk)
            vs.append(vv)
    return ks, vs


def _inputs(dtype, B, H, Hk, N, cap, D, n_new, seed):
    dt = DT[dtype]
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32).to(dt)
    q = rnd(B, H, N, D)
    kc, vc = rnd(B, Hk, cap, D), rnd(B, Hk, cap, D)
    kn = vn = None
    if n_new:
        kn, vn = rnd(B, Hk, n_new, D), rnd(B, Hk, n_new, D)
    return q, kc, vc, kn, vn


# dtype x D x N x causal x Hk: every head dim and dtype, N in {1, 3, 16}, Hk in {H, H/4, 1}
GRID = []
for i, (dtype, D, N) in enumerate([(dt, d, n) for dt in ("bf16", "f16", "f32") for d in (16, 32, 64, 96, 128) for n in (1, 3, 16)]):
    GRID.append((f"{dtype}_d{D}_n{N}", dtype, D, N, i % 2 == 0, (8, 2, 1)[i % 3]))


@pytest.mark.parametrize("name,dtype,D,N,causal,Hk", GRID, ids=[c[0] for c in GRID])
def test_kvcache_grid(name, dtype, D, N, causal, Hk):
    H, B, cap = 8, 3, 300
    n_new = (0, 1, N)[D % 3]
    q, kc, vc, kn, vn = _inputs(dtype, B, H, Hk, N, cap, D, n_new, seed=sum(map(ord, name)))
    seq = [0, 17, cap - n_new] if N == 1 else [5, 130, cap - n_new]
    lens = [s + n_new for s in seq]
    with torch.no_grad():
        o = _api()(q, kc, vc, kn, vn, torch.tensor(seq, dtype=torch.int32, device="cuda"), causal=causal)
    torch.cuda.synchronize()
    ks, vs = _seqs(kc, vc, lens)
    _verify(dtype, o, q, ks, vs, dict(causal=causal), name)
    for b, L in enumerate(lens):
        if L == 0:
            assert (o[b] == 0).all(), (name, b)


# exponent regimes, groups, l2norm off (id, dtype, D, N, H, Hk, kwargs)
REGIMES = [
    ("f16_scale8_groups2_per_row", "f16", 64, 4, 8, 2, dict(scale=8.0, groups=2, causal=True)),
    ("bf16_scale120_per_row", "bf16", 128, 1, 8, 8, dict(scale=120.0)),
    ("f32_scale120_per_row", "f32", 64, 3, 4, 1, dict(scale=120.0, causal=True)),
    ("f16_static_scale4", "f16", 128, 2, 8, 2, dict(scale=4.0)),
    ("bf16_groups4", "bf16", 64, 3, 8, 2, dict(groups=4, scale=2.0, causal=True)),
    ("bf16_groups16_in_lane", "bf16", 64, 1, 4, 4, dict(groups=16, scale=1.0)),
    ("f32_groups8", "f32", 32, 2, 4, 2, dict(groups=8, scale=1.0)),
    ("f16_no_l2norm", "f16", 64, 2, 4, 2, dict(l2norm_qk=False, scale=1.0, causal=True)),
    ("f32_no_l2norm", "f32", 96, 1, 4, 4, dict(l2norm_qk=False, scale=2.0)),
    ("bf16_d96_groups3", "bf16", 96, 2, 4, 2, dict(groups=3, scale=2.0)),
    # D = 96 group widths that straddle a lane's fragment (48, 24, 12, 6, 3 features): the kernel's LDS form
    ("f16_d96_groups2_per_row", "f16", 96, 4, 8, 2, dict(groups=2, scale=8.0, causal=True)),
    ("bf16_d96_groups2", "bf16", 96, 1, 8, 8, dict(groups=2, scale=8.0)),
    ("bf16_d96_groups4", "bf16", 96, 3, 8, 2, dict(groups=4, scale=2.0, causal=True)),
    ("f32_d96_groups4", "f32", 96, 2, 4, 1, dict(groups=4, scale=4.0)),
    ("f16_d96_groups8", "f16", 96, 1, 4, 4, dict(groups=8, scale=1.0)),
    ("f32_d96_groups16_per_row", "f32", 96, 3, 4, 2, dict(groups=16, scale=8.0, causal=True)),
    ("bf16_d96_groups32_per_row", "bf16", 96, 2, 8, 2, dict(groups=32, scale=4.0)),
    ("f16_d96_groups32", "f16", 96, 1, 4, 1, dict(groups=32, scale=0.25)),
]


def _unit_normalised(q, k, groups, l2norm):
    if not l2norm:
        q, k = torch.nn.functional.normalize(q.float(), dim=-1).to(q.dtype), torch.nn.functional.normalize(k.float(), dim=-1).to(k.dtype)
    return q, k


@pytest.mark.parametrize("name,dtype,D,N,H,Hk,kw", REGIMES, ids=[c[0] for c in REGIMES])
def test_kvcache_regimes(name, dtype, D, N, H, Hk, kw):
    B, cap = 2, 700
    q, kc, vc, kn, vn = _inputs(dtype, B, H, Hk, N, cap, D, N, seed=sum(map(ord, name)))
    q, kc = _unit_normalised(q, kc, kw.get("groups", 1), kw.get("l2norm_qk", True))
    if kn is not None:
        _, kn = _unit_normalised(q, kn, 1, kw.get("l2norm_qk", True))
    seq = [600, 33]
    with torch.no_grad():
        o = _api()(q, kc, vc, kn, vn, torch.tensor(seq, dtype=torch.int32, device="cuda"), **kw)
    torch.cuda.synchronize()
    ks, vs = _seqs(kc, vc, [s + N for s in seq])
    _verify(dtype, o, q, ks, vs, kw, name)


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_kvcache_paged_equals_contiguous(dtype):
    B, H, Hk, N, D, page, mb = 3, 8, 2, 2, 64, 32, 6
    cap = page * mb
    q, kc, vc, kn, vn = _inputs(dtype, B, H, Hk, N, cap, D, N, seed=7)
    seq = [0, 70, cap - N]
    # pool: the sequences' pages scattered over a larger pool, in the vLLM [num_blocks, page, Hk, D] layout passed transposed
    nb = B * mb + 5
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(3))[:B * mb].reshape(B, mb).to(torch.int32)
    pool_k = torch.full((nb, page, Hk, D), float("nan"), device="cuda", dtype=DT[dtype])
    pool_v = torch.full_like(pool_k, float("nan"))
    for b in range(B):
        for i in range(mb):
            pool_k[int(perm[b, i])] = kc[b, :, i * page:(i + 1) * page].transpose(0, 1)
            pool_v[int(perm[b, i])] = vc[b, :, i * page:(i + 1) * page].transpose(0, 1)
    kpool, vpool = pool_k.transpose(1, 2), pool_v.transpose(1, 2)
    # untouched pages (not in any table) stay NaN; the contiguous copies get the same append
    sl = torch.tensor(seq, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        oc = _api()(q, kc, vc, kn, vn, sl, causal=True)
        op = _api()(q, kpool, vpool, kn, vn, sl, block_table=perm.cuda(), causal=True)
        oh = _api()(q, kpool, vpool, kn, vn, torch.tensor(seq, dtype=torch.int32), block_table=perm, causal=True)
    torch.cuda.synchronize()
    assert torch.equal(oc, op) and torch.equal(op, oh)
    ks, vs = _seqs(kc, vc, [s + N for s in seq])
    _verify(dtype, op, q, ks, vs, dict(causal=True), f"paged_{dtype}")
    unused = sorted(set(range(nb)) - set(perm.flatten().tolist()))
    assert torch.isnan(pool_k[unused]).all() and torch.isnan(pool_v[unused]).all()
    for b in range(B):
        for t in range(N):
            pos = seq[b] + t
            blk = int(perm[b, pos // page])
            assert torch.equal(pool_k[blk, pos % page], kn[b, :, t]) and torch.equal(pool_v[blk, pos % page], vn[b, :, t])


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_kvcache_append_guard_regions(dtype):
    """A NaN-filled arena around [B, capacity, Hk, D]-transposed caches: the appended slots equal k_new / v_new bit for bit, every other
    slot (valid or not) keeps its bits, the guard bands stay NaN, and the result is finite."""
    B, H, Hk, N, D, cap, guard = 3, 4, 2, 3, 32, 100, 4096
    dt = DT[dtype]
    q, kc0, vc0, kn, vn = _inputs(dtype, B, H, Hk, N, cap, D, N, seed=11)
    arena_k = torch.full((2 * guard + B * cap * Hk * D,), float("nan"), device="cuda", dtype=dt)
    arena_v = torch.full_like(arena_k, float("nan"))
    kc = arena_k[guard:guard + B * cap * Hk * D].view(B, cap, Hk, D).transpose(1, 2)
    vc = arena_v[guard:guard + B * cap * Hk * D].view(B, cap, Hk, D).transpose(1, 2)
    seq = [0, 40, cap - N]
    kc.copy_(kc0)
    vc.copy_(vc0)
    # slots beyond each sequence's length hold NaN: they must never reach the output
    for b, s in enumerate(seq):
        kc[b, :, s:] = float("nan")
        vc[b, :, s:] = float("nan")
    before_k, before_v = kc.clone(), vc.clone()
    with torch.no_grad():
        o = _api()(q, kc, vc, kn, vn, torch.tensor(seq, dtype=torch.int32, device="cuda"), causal=False)
    torch.cuda.synchronize()
    assert torch.isfinite(o).all()
    assert torch.isnan(arena_k[:guard]).all() and torch.isnan(arena_k[-guard:]).all()
    assert torch.isnan(arena_v[:guard]).all() and torch.isnan(arena_v[-guard:]).all()
    exp_k, exp_v = before_k.clone(), before_v.clone()
    for b, s in enumerate(seq):
        exp_k[b, :, s:s + N] = kn[b]
        exp_v[b, :, s:s + N] = vn[b]
    same = lambda a, e: torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32),
                                    e.view(torch.int16 if e.element_size() == 2 else torch.int32))
    assert same(kc.contiguous(), exp_k.contiguous()) and same(vc.contiguous(), exp_v.contiguous())
    ks, vs = _seqs(kc, vc, [s + N for s in seq])
    _verify(dtype, o, q, ks, vs, {}, f"guard_{dtype}")


def test_kvcache_ragged_host_device_int_seqlens():
    B, H, Hk, N, D, cap = 4, 8, 8, 1, 128, 1000
    q, kc, vc, _, _ = _inputs("bf16", B, H, Hk, N, cap, D, 0, seed=5)
    seq = [0, 1, 999, 1000]
    with torch.no_grad():
        od = _api()(q, kc, vc, cache_seqlens=torch.tensor(seq, dtype=torch.int32, device="cuda"), causal=True)
        oh = _api()(q, kc, vc, cache_seqlens=torch.tensor(seq, dtype=torch.int32), causal=True, max_seqlen_k=1000)
        of = _api()(q, kc, vc, causal=True)                         # None: every sequence full
        oi = _api()(q, kc, vc, cache_seqlens=1000, causal=True)
        small = _api()(q, kc, vc, cache_seqlens=torch.tensor(seq, dtype=torch.int32, device="cuda"), causal=True, max_seqlen_k=64)
    torch.cuda.synchronize()
    assert torch.equal(od, oh) and torch.equal(of, oi)
    assert (od[0] == 0).all()
    assert torch.equal(od[3], of[3])
    ks, vs = _seqs(kc, vc, seq)
    _verify("bf16", od, q, ks, vs, dict(causal=True), "ragged")
    # a max_seqlen_k below the true lengths only changes the grid, never the result's meaning
    _verify("bf16", small, q, ks, vs, dict(causal=True), "ragged_small_grid")


@pytest.mark.parametrize("dtype,N,causal,Hk", [("bf16", 1, True, 2), ("f16", 4, True, 8), ("f32", 2, False, 1)])
def test_kvcache_matches_dense_equal_lengths(dtype, N, causal, Hk):
    import flash_cosine_sim_attention_amd as F
    B, H, D, L = 2, 8, 64, 777
    q, kc, vc, _, _ = _inputs(dtype, B, H, Hk, N, 1024, D, 0, seed=9)
    with torch.no_grad():
        o = _api()(q, kc, vc, cache_seqlens=L, causal=causal)
        dense = F.flash_cosine_sim_attention(q, kc[:, :, :L].contiguous(), vc[:, :, :L].contiguous(), causal=causal)
    torch.cuda.synchronize()
    atol, rtol, rel = T.FWD_TOL[dtype]
    assert _rel(_np(o), _np(dense)) <= 2 * rel
    ks, vs = _seqs(kc, vc, [L] * B)
    _verify(dtype, o, q, ks, vs, dict(causal=causal), f"dense_{dtype}")


def test_kvcache_rejects_grad_and_bad_pages():
    q, kc, vc, kn, vn = _inputs("bf16", 1, 2, 2, 1, 64, 32, 1, seed=1)
    with pytest.raises(RuntimeError):
        _api()(q.requires_grad_(), kc, vc, cache_seqlens=3)
    q = q.detach()
    with pytest.raises(ValueError):
        _api()(q, kc[:, :, :24], vc[:, :, :24], block_table=torch.zeros(1, 2, dtype=torch.int32), cache_seqlens=3)


def test_kvcache_opcheck():
    import flash_cosine_sim_attention_amd._torch_ops as ops
    fc = ops.load()
    q, kc, vc, kn, vn = _inputs("bf16", 2, 4, 2, 2, 64, 32, 2, seed=2)
    sl = torch.tensor([3, 40], dtype=torch.int32, device="cuda")
    torch.library.opcheck(fc.kvcache_forward.default, (q, kc, vc, kn, vn, sl, None, 64, 8.0, True, True, 1))
    tab = torch.tensor([[1, 0], [2, 3]], dtype=torch.int32, device="cuda")
    kp, vp = torch.randn(4, 2, 32, 32, device="cuda", dtype=torch.bfloat16), torch.randn(4, 2, 32, 32, device="cuda", dtype=torch.bfloat16)
    torch.library.opcheck(fc.kvcache_forward.default, (q, kp, vp, kn, vn, sl, tab, 64, 8.0, False, True, 1))


def test_kvcache_graph_capture_and_replay():
    B, H, Hk, N, D, cap = 2, 8, 2, 1, 64, 512
    q, kc, vc, kn, vn = _inputs("bf16", B, H, Hk, N, cap, D, 1, seed=4)
    sl = torch.tensor([10, 300], dtype=torch.int32, device="cuda")
    f = _api()
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            f(q, kc, vc, kn, vn, sl, max_seqlen_k=cap)              # warm-up (allocator, lazy init)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        kc_eager, vc_eager = kc.clone(), vc.clone()               # the caches after the warm-up's append
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = f(q, kc, vc, kn, vn, sl, max_seqlen_k=cap)
        for step in range(3):
            q.copy_(torch.randn_like(q))
            kn.copy_(torch.randn_like(kn))
            vn.copy_(torch.randn_like(vn))
            sl.copy_(torch.tensor([11 + step, 301 + 2 * step], dtype=torch.int32))
            g.replay()
            ref = f(q, kc_eager, vc_eager, kn, vn, sl, max_seqlen_k=cap)
            torch.cuda.synchronize()
            assert torch.equal(out, ref), step
            assert torch.equal(kc, kc_eager) and torch.equal(vc, vc_eager), step


@pytest.mark.parametrize("dtype,D", [("bf16", 32), ("f16", 16), ("f32", 32)])
def test_kvcache_many_splits_long_cache(dtype, D):
    """A long cache on a small grid: tens of key splits (decode_splits), windows that end inside a 32-key block, ragged lengths; the combine
    reconciles every split, in the static regime and (float16 at scale 16, groups 2) the per-row regime."""
    B, H, Hk, N, cap = 3, 4, 1, 3, 20000
    q, kc, vc, kn, vn = _inputs(dtype, B, H, Hk, N, cap, D, 2, seed=D + len(dtype))
    seq = [cap - 2, 7775, 553]
    for kw in (dict(causal=True), dict(scale=16.0, groups=2)):
        kc_, vc_ = kc.clone(), vc.clone()
        with torch.no_grad():
            o = _api()(q, kc_, vc_, kn, vn, torch.tensor(seq, dtype=torch.int32, device="cuda"), **kw)
        torch.cuda.synchronize()
        ks, vs = _seqs(kc_, vc_, [s + 2 for s in seq])
        _verify(dtype, o, q, ks, vs, kw, f"splits_{dtype}_d{D}_{sorted(kw)}")
