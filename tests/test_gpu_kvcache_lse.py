"""The decode calls' log-sum-exp and the merge of attention states on the GPU (return_lse=True of flash_cosine_sim_attention_with_kvcache
and flash_cosine_sim_attention_varlen_with_kvcache; merge_attention_states; fcsa_forward_kvcache_lse, fcsa_merge_states).

return_lse changes nothing else: o and the caches after the append equal the call without it bit for bit on every route.  lse[row] is
log(sum over the row's visible keys of exp(logit)), -inf exactly for a row without a visible key, the same in both exponent regimes.  It
is compared twice (tests/tolerances_lse.py): against float64 on the raw inputs with a derived bound, and against float64 on the operands
the kernel is fed with a measured one.  The merge kernel is compared with the float64 merge of its own inputs, and one attention cut over
two or three calls with the float64 oracle on the whole problem."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases as CS
import tolerances as T
import tolerances_lse as TL
import lse_reference as R
import test_gpu_kvcache as TK
import test_gpu_kvcache_fp8 as TF

pytestmark = pytest.mark.gpu

DT = TK.DT
NEG_INF = float("-inf")


def _F():
    import flash_cosine_sim_attention_amd as F
    return F


def _np(t):
    return t.detach().cpu().double().numpy()


def _lse_ref(q, kseq, kw, operand_dtype=None, window=(-1, -1)):
    """[B, H, N] float64: lse_reference.lse_rows per sequence; kseq: list of [Hk, L_b, D] (torch or float64 numpy)"""
    okw = dict(scale=kw.get("scale", 8.0), groups=kw.get("groups", 1), causal=kw.get("causal", False), l2norm_qk=kw.get("l2norm_qk", True))
    return np.stack([R.lse_rows(_np(q[b]), _np(k) if isinstance(k, torch.Tensor) else k, operand_dtype=operand_dtype, window=window, **okw)
                     for b, k in enumerate(kseq)])


def check_lse(dtype, lse, q, kseq, kw, label, window=(-1, -1)):
    """-inf exactly where the reference is (and nowhere else, no NaN), the derived bound against the raw inputs and the measured bar against
    the operands the kernel is fed (16-bit with l2norm_qk: the rounded ones)."""
    assert lse.dtype == torch.float32 and not torch.isnan(lse).any(), label
    got = _np(lse)
    raw = _lse_ref(q, kseq, kw, None, window)
    empty = np.isneginf(raw)
    assert np.array_equal(np.isneginf(got), empty), label
    assert np.isfinite(got[~empty]).all(), label
    scale, groups, l2 = kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True)
    d_raw = float(np.abs(got[~empty] - raw[~empty]).max(initial=0.0))
    bound = R.derived_lse_bound(dtype, scale, groups, l2)
    assert T.check(label + "/lse-raw", dtype, d_raw, bound), (label, d_raw, bound)
    ops = _lse_ref(q, kseq, kw, dtype, window) if (dtype != "f32" and l2) else raw
    d_ops = float(np.abs(got[~empty] - ops[~empty]).max(initial=0.0))
    assert T.check(label + "/lse-operands", dtype, d_ops, TL.LSE_TOL[dtype]), (label, d_ops, TL.LSE_TOL[dtype])
    return empty


# ---- 1. the grid: every dtype x D x N, G * N crossing the 16-row tile; o and the caches bit for bit, -inf rows, finite elsewhere ----------
GRID = []
for i, (dtype, D, N) in enumerate([(dt, d, n) for dt in ("bf16", "f16", "f32") for d in (16, 32, 64, 96, 128) for n in (1, 3, 16)]):
    # Hk cycles against N (the innermost index), so G * N takes 1, 4, 8, 3, 12, 24, 16, 64 and 128: below a tile, a partial second tile, whole tiles
    GRID.append((f"{dtype}_d{D}_n{N}", dtype, D, N, i % 2 == 0, (8, 2, 1)[(i // 3 + i) % 3]))


@pytest.mark.parametrize("name,dtype,D,N,causal,Hk", GRID, ids=[c[0] for c in GRID])
def test_lse_grid(name, dtype, D, N, causal, Hk):
    f = _F().flash_cosine_sim_attention_with_kvcache
    H, B, cap = 8, 3, 300
    lens = [5 if N == 16 else 0, 130, 300]
    n_new = (0, 1, 3)[D % 3] if N == 16 else 0             # (an append needs a slot: the empty sequence has none to fill and stay empty)
    q, kc, vc, kn, vn = TK._inputs(dtype, B, H, Hk, N, cap, D, n_new, seed=sum(map(ord, name)))
    sl = torch.tensor([L - n_new for L in lens], dtype=torch.int32, device="cuda")
    kc2, vc2 = kc.clone(), vc.clone()
    with torch.no_grad():
        o_plain = f(q, kc2, vc2, kn, vn, sl, causal=causal)
        o, lse = f(q, kc, vc, kn, vn, sl, causal=causal, return_lse=True)
    torch.cuda.synchronize()
    assert TK_bits_equal(o, o_plain) and TK_bits_equal(kc, kc2) and TK_bits_equal(vc, vc2), name
    assert lse.shape == (B, H, N)
    ks, _ = TK._seqs(kc, vc, lens)
    empty = check_lse(dtype, lse, q, ks, dict(causal=causal), name)
    if N != 16:
        assert empty[0].all() and (lse[0] == NEG_INF).all() and (o[0] == 0).all()
    elif causal:                                          # 5 keys, 16 queries: rows 0 .. N - 6 see nothing
        assert (lse[0, :, :N - 5] == NEG_INF).all() and torch.isfinite(lse[0, :, N - 5:]).all()
        assert (o[0, :, :N - 5] == 0).all()
    assert torch.isfinite(lse[1:]).all()


def TK_bits_equal(a, b):
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


# ---- 3. many splits: tens of splits, the last window ending inside a 32-key block; both exponent regimes ----------------------------------
@pytest.mark.parametrize("dtype,D,kw", [("bf16", 64, dict(scale=8.0)), ("bf16", 128, dict(scale=8.0)),
                                        ("f16", 64, dict(scale=16.0, groups=2)), ("f16", 128, dict(scale=16.0, groups=2))],
                         ids=["bf16_d64_static", "bf16_d128_static", "f16_d64_per_row", "f16_d128_per_row"])
def test_lse_many_splits(dtype, D, kw):
    f = _F().flash_cosine_sim_attention_with_kvcache
    B, H, Hk, N, L, cap = 1, 4, 1, 3, 5003, 5120
    assert CS.dynamic_shift_regime(dtype, kw["scale"], kw.get("groups", 1), True, False) == (dtype == "f16")
    q, kc, vc, _, _ = TK._inputs(dtype, B, H, Hk, N, cap, D, 0, seed=D + len(dtype))
    sl = torch.tensor([L], dtype=torch.int32, device="cuda")
    with torch.no_grad():
        o_plain = f(q, kc, vc, cache_seqlens=sl, causal=True, **kw)
        o, lse = f(q, kc, vc, cache_seqlens=sl, causal=True, return_lse=True, **kw)
    torch.cuda.synchronize()
    assert TK_bits_equal(o, o_plain)
    ks, _ = TK._seqs(kc, vc, [L])
    check_lse(dtype, lse, q, ks, dict(causal=True, **kw), f"splits_{dtype}_d{D}")


# ---- 4. one case per remaining route ---------------------------------------------------------------------------------------------------------
def test_lse_paged_shuffled_table():
    f = _F().flash_cosine_sim_attention_with_kvcache
    dtype, B, H, Hk, N, D, page, mb = "bf16", 3, 8, 2, 2, 64, 16, 12
    cap = page * mb
    q, kc, vc, kn, vn = TK._inputs(dtype, B, H, Hk, N, cap, D, N, seed=21)
    seq = [0, 70, cap - N]
    nb = B * mb + 5
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(3))[:B * mb].reshape(B, mb).to(torch.int32)
    kpool = torch.full((nb, Hk, page, D), float("nan"), device="cuda", dtype=DT[dtype])
    vpool = torch.full_like(kpool, float("nan"))
    for b in range(B):
        for i in range(mb):
            kpool[int(perm[b, i])] = kc[b, :, i * page:(i + 1) * page]
            vpool[int(perm[b, i])] = vc[b, :, i * page:(i + 1) * page]
    sl, tab = torch.tensor(seq, dtype=torch.int32, device="cuda"), perm.cuda()
    kp2, vp2 = kpool.clone(), vpool.clone()
    with torch.no_grad():
        o_plain = f(q, kp2, vp2, kn, vn, sl, block_table=tab, causal=True)
        o, lse = f(q, kpool, vpool, kn, vn, sl, block_table=tab, causal=True, return_lse=True)
        f(q, kc, vc, kn, vn, sl, causal=True)                  # the contiguous copies get the same append: the reference's keys
    torch.cuda.synchronize()
    assert TK_bits_equal(o, o_plain) and TK_bits_equal(kpool, kp2) and TK_bits_equal(vpool, vp2)
    ks, _ = TK._seqs(kc, vc, [s + N for s in seq])
    check_lse(dtype, lse, q, ks, dict(causal=True), "paged")


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_lse_window(dtype):
    f = _F().flash_cosine_sim_attention_with_kvcache
    B, H, Hk, N, D, cap = 3, 8, 2, 3, 64, 300
    q, kc, vc, kn, vn = TK._inputs(dtype, B, H, Hk, N, cap, D, N, seed=31)
    seq = [0, 130, cap - N]
    sl = torch.tensor(seq, dtype=torch.int32, device="cuda")
    kc2, vc2 = kc.clone(), vc.clone()
    with torch.no_grad():
        o_plain = f(q, kc2, vc2, kn, vn, sl, window_size=(40, 0))
        o, lse = f(q, kc, vc, kn, vn, sl, window_size=(40, 0), return_lse=True)
    torch.cuda.synchronize()
    assert TK_bits_equal(o, o_plain) and TK_bits_equal(kc, kc2)
    ks, _ = TK._seqs(kc, vc, [s + N for s in seq])
    check_lse(dtype, lse, q, ks, {}, f"window_{dtype}", window=(40, 0))


@pytest.mark.parametrize("l2norm", [True, False], ids=["l2norm", "no_l2norm"])
def test_lse_fp8_cache(l2norm):
    f = _F().flash_cosine_sim_attention_with_kvcache
    dtype, B, H, Hk, N, D, cap = "f16", 3, 8, 2, 2, 64, 300
    kw = dict(causal=True) if l2norm else dict(causal=True, l2norm_qk=False, scale=1.0)
    q, kc, vc, kn, vn = TK._inputs(dtype, B, H, Hk, N, cap, D, N, seed=41)
    q, kc = TK._unit_normalised(q, kc, 1, l2norm)
    _, kn = TK._unit_normalised(q, kn, 1, l2norm)
    (k8, ks), (v8, vs) = TF._quantise(kc), TF._quantise(vc)
    assert ks.shape == (B, Hk) and float((ks - 1).abs().min()) > 0
    seq = [0, 130, cap - N]
    sl = torch.tensor(seq, dtype=torch.int32, device="cuda")
    k82, v82 = k8.clone(), v8.clone()
    with torch.no_grad():
        o_plain = f(q, k82, v82, kn, vn, sl, k_scale=ks, v_scale=vs, **kw)
        o, lse = f(q, k8, v8, kn, vn, sl, k_scale=ks, v_scale=vs, return_lse=True, **kw)
    torch.cuda.synchronize()
    assert TK_bits_equal(o, o_plain) and TK_bits_equal(k8.view(torch.uint8), k82.view(torch.uint8)) and TK_bits_equal(v8.view(torch.uint8), v82.view(torch.uint8))
    kseq, _ = TF._seqs(k8, v8, ks, vs, [s + N for s in seq])      # the values the codes mean: k_scale inside, v_scale nowhere near
    check_lse(dtype, lse, q, [k.cpu().numpy() for k in kseq], kw, f"fp8_{'l2norm' if l2norm else 'raw'}")


@pytest.mark.parametrize("dtype,fp8", [("bf16", False), ("f32", False), ("f16", True)], ids=["bf16", "f32", "f16_fp8"])
def test_lse_ragged(dtype, fp8):
    f = _F().flash_cosine_sim_attention_varlen_with_kvcache
    counts, cached, H, Hk, D, cap = [1, 0, 4, 17], [0, 17, 130, 5], 8, 2, 64, 300
    B, total = len(counts), sum(counts)
    g = torch.Generator(device="cuda").manual_seed(51)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32).to(DT[dtype])
    q, kn, vn, kc, vc = rnd(total, H, D), rnd(total, Hk, D), rnd(total, Hk, D), rnd(B, Hk, cap, D), rnd(B, Hk, cap, D)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device="cuda")
    sl = torch.tensor(cached, dtype=torch.int32, device="cuda")
    quant = {}
    if fp8:
        (kc, ks), (vc, vs) = TF._quantise(kc), TF._quantise(vc)
        quant = dict(k_scale=ks, v_scale=vs)
    kc2, vc2 = kc.clone(), vc.clone()
    with torch.no_grad():
        o_plain = f(q, kc2, vc2, cu, kn, vn, sl, causal=True, **quant)
        o, lse = f(q, kc, vc, cu, kn, vn, sl, causal=True, return_lse=True, **quant)
    torch.cuda.synchronize()
    as_bytes = (lambda t: t.view(torch.uint8)) if fp8 else (lambda t: t)
    assert TK_bits_equal(o, o_plain) and TK_bits_equal(as_bytes(kc), as_bytes(kc2)) and TK_bits_equal(as_bytes(vc), as_bytes(vc2))
    assert lse.shape == (total, H) and lse.dtype == torch.float32
    lens = [c + n for c, n in zip(cached, counts)]
    if fp8:
        kseq = [k.cpu().numpy() for k in TF._seqs(kc, vc, ks, vs, lens)[0]]
    else:
        kseq = TK._seqs(kc, vc, lens)[0]
    c = cu.tolist()
    for b in range(B):
        if counts[b] == 0:
            continue
        qb = q[c[b]:c[b + 1]].permute(1, 0, 2).unsqueeze(0)                         # [1, H, N_b, D]
        lb = lse[c[b]:c[b + 1]].permute(1, 0).unsqueeze(0)
        check_lse(dtype, lb, qb, [kseq[b]], dict(causal=True), f"ragged_{dtype}_seq{b}")


def test_lse_non_contiguous_q():
    f = _F().flash_cosine_sim_attention_with_kvcache
    dtype, B, H, Hk, N, D, cap = "bf16", 2, 8, 2, 3, 64, 200
    _, kc, vc, _, _ = TK._inputs(dtype, B, H, Hk, N, cap, D, 0, seed=61)
    qkv = torch.randn(B, N, 3, H, D, device="cuda", dtype=DT[dtype])
    q = qkv[:, :, 0].transpose(1, 2)                                             # [B, H, N, D], a strided view of a packed projection
    assert not q.is_contiguous()
    sl = torch.tensor([77, 200], dtype=torch.int32, device="cuda")
    with torch.no_grad():
        o_plain = f(q, kc, vc, cache_seqlens=sl)
        o, lse = f(q, kc, vc, cache_seqlens=sl, return_lse=True)
        o_c, lse_c = f(q.contiguous(), kc, vc, cache_seqlens=sl, return_lse=True)
    torch.cuda.synchronize()
    assert TK_bits_equal(o, o_plain) and TK_bits_equal(o, o_c) and TK_bits_equal(lse, lse_c)
    check_lse(dtype, lse, q, TK._seqs(kc, vc, [77, 200])[0], {}, "strided_q")


# ---- 5. the merge kernel against the float64 merge of its own inputs -----------------------------------------------------------------------
def _states(dtype, shape, S, seed, empty_rows=True):
    g = torch.Generator(device="cuda").manual_seed(seed)
    os = [torch.randn(*shape, device="cuda", generator=g, dtype=torch.float32).to(DT[dtype]) for _ in range(S)]
    lses = [4 * torch.randn(*shape[:-1], device="cuda", generator=g, dtype=torch.float32) for _ in range(S)]
    if empty_rows:       # some empty states, with NaN in their o, and a few rows where every state is empty
        for s in range(S):
            hole = torch.rand(*shape[:-1], device="cuda", generator=g) < 0.15
            lses[s][hole] = NEG_INF
            os[s][hole] = float("nan")
        lses[0].view(-1)[:2] = NEG_INF
        for s in range(S):
            lses[s].view(-1)[2:4] = NEG_INF
            os[s].view(-1, shape[-1])[2:4] = float("nan")
    return os, lses


def check_merge(dtype, o, lse, os, lses, label):
    ro, rl = R.merge_reference([_np(t) for t in os], [_np(t) for t in lses])
    go, gl = _np(o), _np(lse)
    assert not torch.isnan(o).any() and not torch.isnan(lse).any(), label
    dead = np.isneginf(rl)
    assert np.array_equal(np.isneginf(gl), dead) and (go[dead] == 0).all(), label
    live = [np.where(np.isfinite(_np(l))[..., None], np.abs(np.nan_to_num(_np(t))), 0.0) for t, l in zip(os, lses)]
    omax = np.max(np.stack(live), axis=0).max(axis=-1, keepdims=True)
    excess = float((np.abs(go - ro) - R.ULP[dtype] * np.abs(ro) - 2.0 ** -20 * omax).max(initial=0.0))
    assert T.check(label + "/merge-o-excess", dtype, excess, 0.0), (label, excess)
    d = float(np.abs(gl[~dead] - rl[~dead]).max(initial=0.0))
    assert T.check(label + "/merge-lse", dtype, d, TL.MERGE_LSE_TOL), (label, d)


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("D", [16, 128])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
def test_merge_against_float64(dtype, D, S):
    merge = _F().merge_attention_states
    shape = (3, 5, 7, D)                                   # 105 rows: no multiple of the 256-thread block at either D
    os, lses = _states(dtype, shape, S, seed=S * 1000 + D)
    o, lse = merge(os, lses)
    torch.cuda.synchronize()
    assert o.shape == shape and o.is_contiguous() and lse.shape == shape[:-1] and lse.is_contiguous() and lse.dtype == torch.float32
    check_merge(dtype, o, lse, os, lses, f"merge_{dtype}_d{D}_s{S}")
    o2, lse2 = merge(os, lses)
    assert TK_bits_equal(o, o2) and TK_bits_equal(lse, lse2)                      # deterministic
    # the packed 3-D form reads the same rows
    o3, lse3 = merge([t.flatten(0, 1) for t in os], [t.flatten(0, 1) for t in lses])
    assert TK_bits_equal(o3, o.flatten(0, 1)) and TK_bits_equal(lse3, lse.flatten(0, 1))


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_merge_identities(dtype):
    merge = _F().merge_attention_states
    shape = (2, 4, 9, 64)
    (a,), (la,) = _states(dtype, shape, 1, seed=7, empty_rows=False)
    a.view(-1)[::5] = -0.0
    o, lse = merge([a], [la])
    assert TK_bits_equal(o, a) and TK_bits_equal(lse, la)                         # one state: bit for bit
    nan_o, empty = torch.full_like(a, float("nan")), torch.full_like(la, NEG_INF)
    for os, lses in (([a, nan_o], [la, empty]), ([nan_o, a], [empty, la]), ([nan_o, a, nan_o], [empty, la, empty])):
        o, lse = merge(os, lses)
        assert TK_bits_equal(o, a) and TK_bits_equal(lse, la)                     # beside empty states: bit for bit
    o, lse = merge([nan_o, nan_o], [empty, empty])
    assert (o == 0).all() and (lse == NEG_INF).all()                              # every state empty


@pytest.mark.parametrize("dtype,D", [("bf16", 16), ("f16", 128), ("f32", 16)])
def test_merge_strided_inputs_and_guarded_outputs(dtype, D):
    """fcsa_merge_states over strided views of the inputs (a [B, N, H, D] buffer read as [B, H, N, D], an lse stored [H, B, N]) and
    outputs that sit inside NaN arenas: the guard bands around them stay NaN, the result equals the public call on contiguous copies."""
    from flash_cosine_sim_attention_amd import _lib
    lib = _lib.load()
    B, H, N, S, guard = 2, 3, 5, 3, 1024
    os_c, lses_c = _states(dtype, (B, H, N, D), S, seed=D + 5)
    os = [t.transpose(1, 2).contiguous().transpose(1, 2) for t in os_c]            # [B, H, N, D] views of [B, N, H, D] storage
    lses = [t.permute(1, 0, 2).contiguous().permute(1, 0, 2) for t in lses_c]      # [B, H, N] views of [H, B, N] storage
    assert not os[0].is_contiguous() and not lses[0].is_contiguous()
    rows = B * H * N
    arena_o = torch.full((2 * guard + rows * D,), float("nan"), device="cuda", dtype=DT[dtype])
    arena_l = torch.full((2 * guard + rows,), float("nan"), device="cuda", dtype=torch.float32)
    o, lse = arena_o[guard:guard + rows * D].view(B, H, N, D), arena_l[guard:guard + rows].view(B, H, N)
    a = _lib.MergeArgs()
    a.dtype, a.size0, a.size1, a.size2, a.dim_head, a.states = _lib.dtype_code(DT[dtype]), B, H, N, D, S
    for s in range(S):
        a.o_in[s] = _lib.tensor4(os[s])
        a.lse_in[s] = _lib.LseOut(lses[s].data_ptr(), *lses[s].stride())
    a.o = _lib.tensor4(o)
    a.lse = _lib.LseOut(lse.data_ptr(), *lse.stride())
    a.stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.fcsa_merge_states(C.byref(a)), "fcsa_merge_states")
    torch.cuda.synchronize()
    for arena in (arena_o, arena_l):
        assert torch.isnan(arena[:guard]).all() and torch.isnan(arena[-guard:]).all()
    check_merge(dtype, o, lse, os_c, lses_c, f"merge_strided_{dtype}_d{D}")
    o_pub, lse_pub = _F().merge_attention_states(os, lses)                       # the public call reads the same strided views in place
    assert TK_bits_equal(o_pub, o) and TK_bits_equal(lse_pub, lse)


# ---- 6. one attention over two (three) calls -------------------------------------------------------------------------------------------------
def check_composed(dtype, o, q, kseq, vseq, kw, label):
    """the parity policy of test_gpu_kvcache._verify with the composed route's own measured bars (tolerances_lse.COMPOSED_FWD_TOL)"""
    atol, rtol, rel = TL.COMPOSED_FWD_TOL[dtype]
    cond = CS.logit_cond(dtype, kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True))
    refs = [("raw", TK._reference(q, kseq, vseq, kw), cond)]
    if dtype != "f32" and kw.get("l2norm_qk", True):
        refs.append(("operands", TK._reference(q, kseq, vseq, kw, operand_dtype=dtype), 1.0))
    go = _np(o)
    assert torch.isfinite(o).all(), label
    for tag, ref, c in refs:
        assert T.check(f"{label}/{tag}/composed-excess", dtype, float((np.abs(go - ref) - rtol * np.abs(ref)).max(initial=0.0)), atol * c), (label, tag)
        assert T.check(f"{label}/{tag}/composed-rel", dtype, TK._rel(go, ref), rel * c), (label, tag, TK._rel(go, ref), rel * c)
    return TK._rel(go, refs[-1][1])


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("cuts", [(1,), (32,), (77,), (149,), (32, 77)], ids=lambda c: "cut" + "_".join(map(str, c)))
def test_one_attention_over_several_calls(dtype, causal, cuts):
    F = _F()
    f = F.flash_cosine_sim_attention_with_kvcache
    B, H, Hk, N, D, L, cap = 2, 8, 2, 2, 64, 150, 160      # (N = 2: under causal every query sees the whole first part for every cut <= L - N + 1)
    q, kc, vc, _, _ = TK._inputs(dtype, B, H, Hk, N, cap, D, 0, seed=71 + len(cuts))
    edges = [0, *cuts, L]
    with torch.no_grad():
        whole, lse_whole = f(q, kc, vc, cache_seqlens=L, causal=causal, return_lse=True)
        os, lses = [], []
        for lo, hi in zip(edges[:-1], edges[1:]):
            last = hi == L                                  # the queries are the last N positions: only the last part is causal
            o_s, l_s = f(q, kc[:, :, lo:hi], vc[:, :, lo:hi], causal=causal and last, return_lse=True)
            os.append(o_s)
            lses.append(l_s)
        # (the first part through cache_seqlens on the whole cache: the same keys as the view)
        o_first, l_first = f(q, kc, vc, cache_seqlens=edges[1], causal=False, return_lse=True)
        assert TK_bits_equal(o_first, os[0]) and TK_bits_equal(l_first, lses[0])
        o, lse = F.merge_attention_states(os, lses)
    torch.cuda.synchronize()
    ks, vs = TK._seqs(kc, vc, [L] * B)
    label = f"cut_{dtype}_{'causal' if causal else 'full'}_{'_'.join(map(str, cuts))}"
    composed = check_composed(dtype, o, q, ks, vs, dict(causal=causal), label)
    TK._verify(dtype, whole, q, ks, vs, dict(causal=causal), label + "/single")
    ref = TK._reference(q, ks, vs, dict(causal=causal), operand_dtype=None if dtype == "f32" else dtype)
    single = TK._rel(_np(whole), ref)
    T.check(label + "/composed-over-single", dtype, composed / max(single, 1e-12), 2.0)
    assert composed <= 2.0 * single + 1e-7, (label, composed, single)        # more than twice the single call's error: a bug to find
    check_lse(dtype, lse, q, ks, dict(causal=causal), label + "/merged")
    d = float((lse - lse_whole).abs().max())
    assert T.check(label + "/merged-vs-whole-lse", dtype, d, TL.LSE_TOL[dtype]), (label, d)


# ---- 8. opcheck of the new ops' fake kernels ---------------------------------------------------------------------------------------------------
def test_lse_and_merge_opcheck():
    import flash_cosine_sim_attention_amd._torch_ops as ops
    fc = ops.load()
    q, kc, vc, kn, vn = TK._inputs("bf16", 2, 4, 2, 2, 64, 32, 2, seed=2)
    sl = torch.tensor([3, 40], dtype=torch.int32, device="cuda")
    torch.library.opcheck(fc.kvcache_lse_forward.default, (q, kc, vc, None, kn, vn, sl, None, None, None, 0, 64, 8.0, True, True, 1, -1, -1))
    torch.library.opcheck(fc.kvcache_lse_forward.default, (q, kc, vc, None, kn, vn, sl, None, None, None, 0, 64, 8.0, False, True, 1, 20, 0))
    cu = torch.tensor([0, 1, 4], dtype=torch.int32, device="cuda")
    qp, knp, vnp = (torch.randn(4, h, 32, device="cuda", dtype=torch.bfloat16) for h in (4, 2, 2))
    torch.library.opcheck(fc.kvcache_lse_forward.default, (qp, kc, vc, cu, knp, vnp, sl, None, None, None, 3, 64, 8.0, True, True, 1, -1, -1))
    os, lses = _states("bf16", (2, 4, 3, 32), 3, seed=3, empty_rows=False)
    torch.library.opcheck(fc.merge_states.default, (os, lses))
    torch.library.opcheck(fc.merge_states.default, ([t.flatten(0, 1) for t in os], [t.flatten(0, 1) for t in lses]))
