"""tests/fullsize_reference.py proven on the CPU before it judges a kernel.

  * `attention_slice` (torch float64, row blocks restricted to the band) against the numpy oracle -- attention_forward_stats /
    attention_backward with the window as a 0 / -inf attn_bias -- on small problems: every window side open and closed, N < M, N > M, rows
    without a visible key, Hk < H, groups > 1, l2norm_qk = False, both shift regimes, both operand dtypes.  The bar is the one of the
    existing pin (test_gpu_fullsize.py::test_operand_faithful_helper_equals_the_numpy_oracle): 1e-9 * max(1, max|ref|).
  * the exact probes: their closed forms (o and dv) against the oracle, and their forward against this package's CPU path through the
    three public functions (dense window, packed, kvcache): zero pattern with ==, non-zero values within one output ulp relative.
  * test_probe_notices_*: a mistake on the EXPECTATION side -- left off by one, two block-table entries swapped, a packed sequence's offset
    off by one row -- makes the probe comparison fail.  The kernels are never mutated; this shows the probes discriminate.

What the probes do not see: every valid K row is the same vector, so a mis-addressed VALID K row goes unnoticed (random-data slices and the
bit-for-bit address tests cover that); and in 16-bit types a wrong key COUNT in a wide window is below one output ulp unless a sentinel
sits on the affected position -- which is why the float32 probe runs too, where 1 / n_i resolves every count.
"""
import numpy as np
import pytest
import torch

import cases as GC
import fullsize_reference as FR
import tolerances as T
from oracle import cosine_sim_oracle as O


def band(N, M, left, right, causal):
    """the window as an additive bias [1, N, M]: 0 inside the band, -inf outside (as test_gpu_window.py builds it)"""
    i = np.arange(N)[:, None] + (M - N)
    j = np.arange(M)[None]
    ok = np.ones((N, M), bool)
    if left >= 0:
        ok &= j >= i - left
    r = 0 if causal else right
    if r >= 0:
        ok &= j <= i + r
    return np.where(ok, 0.0, -np.inf)[None]


def _np(t):
    return t.detach().double().numpy()


# id, dtype of the inputs, D, G, N, M, window, kwargs, operand dtype
PIN = [
    ("open_open", "f32", 32, 1, 50, 70, (-1, -1), dict(), None),
    ("open_open_causal", "bf16", 32, 2, 70, 70, (-1, -1), dict(causal=True), "bf16"),
    ("left_closed_right_open", "f16", 32, 2, 60, 90, (17, -1), dict(), "f16"),
    ("left_open_right_closed", "bf16", 64, 1, 90, 60, (-1, 5), dict(), None),
    ("both_closed_n_lt_m", "f16", 32, 4, 50, 131, (20, 9), dict(), None),
    ("both_closed_n_gt_m_rows_without_key", "bf16", 32, 2, 131, 50, (20, 9), dict(), "bf16"),
    ("causal_window_n_gt_m_rows_without_key", "f32", 16, 2, 100, 40, (7, 0), dict(causal=True), None),
    ("zero_width", "bf16", 32, 1, 40, 40, (0, 0), dict(), "bf16"),
    ("groups4_static", "bf16", 64, 2, 80, 80, (30, 0), dict(groups=4, scale=2.0, causal=True), "bf16"),
    ("groups2_per_row_f16", "f16", 32, 2, 66, 80, (25, 3), dict(groups=2, scale=8.0), "f16"),
    ("per_row_bf16_scale80", "bf16", 64, 1, 77, 77, (33, -1), dict(scale=80.0), "bf16"),
    ("per_row_f32_scale80", "f32", 32, 2, 77, 60, (-1, 2), dict(scale=80.0), None),
    ("no_l2norm", "f16", 32, 2, 70, 90, (40, 1), dict(l2norm_qk=False, scale=1.0), "f16"),
    ("no_l2norm_causal_raw", "bf16", 32, 1, 70, 70, (10, 0), dict(l2norm_qk=False, scale=1.0, causal=True), None),
    ("several_row_blocks", "bf16", 16, 2, 300, 333, (70, 40), dict(), "bf16"),
]


@pytest.mark.parametrize("name,dtype,D,G,N,M,window,kw,opd", PIN, ids=[c[0] for c in PIN])
@pytest.mark.parametrize("saved", [False, True], ids=["exact_o", "saved_o"])
def test_attention_slice_equals_the_numpy_oracle(name, dtype, D, G, N, M, window, kw, opd, saved):
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    rnd = lambda *s: torch.randn(*s, generator=g).to(FR.DT[dtype])
    q, k, v, do = rnd(G, N, D), rnd(M, D), rnd(M, D), rnd(G, N, D)
    scale, groups, l2, causal = kw.get("scale", 8.0), kw.get("groups", 1), kw.get("l2norm_qk", True), kw.get("causal", False)
    if not l2:
        q, k = (torch.nn.functional.normalize(t.float(), dim=-1).to(FR.DT[dtype]) for t in (q, k))
    dyn = GC.dynamic_shift_regime(dtype, scale, groups, l2, False)
    eps = 1e-300 if dyn else 1e-10
    o_saved = rnd(G, N, D) if saved else None          # (any tensor: delta must be taken from it on both sides)
    got = FR.attention_slice(q, k, v, do, scale=scale, groups=groups, causal=causal, window=window, l2norm_qk=l2, eps=eps,
                             operand_dtype=None if opd is None else FR.DT[opd], o_saved=o_saved, row_block=64)
    fwd_only = FR.attention_slice(q, k, v, scale=scale, groups=groups, causal=causal, window=window, l2norm_qk=l2, eps=eps,
                                  operand_dtype=None if opd is None else FR.DT[opd], row_block=37)
    okw = dict(scale=scale, groups=groups, causal=causal, l2norm_qk=l2, eps=eps, operand_dtype=opd,
               attn_bias=np.repeat(band(N, M, *window, causal), G, axis=0))
    nq, ndo = _np(q)[None], _np(do)[None]
    nk, nv = (np.repeat(_np(t)[None, None], G, axis=1) for t in (k, v))
    ro, _ = O.attention_forward_stats(nq, nk, nv, **okw)
    rdq, rdk, rdv, _ = O.attention_backward(ndo, nq, nk, nv, o_saved=None if o_saved is None else _np(o_saved)[None], **okw)
    refs = (ro[0], rdq[0], rdk[0].sum(0), rdv[0].sum(0))
    for nm, a, r in zip(("o", "dq", "dk", "dv"), got, refs):
        err = np.abs(_np(a) - r).max()
        assert err <= 1e-9 * max(1.0, np.abs(r).max()), (name, nm, err)
    assert np.abs(_np(fwd_only) - ro[0]).max() <= 1e-9 * max(1.0, np.abs(ro).max())
    no_key = (band(N, M, *window, causal)[0] == 0).sum(axis=1) == 0
    if name.endswith("rows_without_key"):
        assert no_key.any()
    assert (_np(got[0])[:, no_key] == 0).all() and (_np(got[1])[:, no_key] == 0).all()


def test_moved_operand_faithful_helper_equals_the_numpy_oracle():
    """grads_operand_faithful as test_gpu_fullsize.py calls it (key mask, no clamp), here on the CPU"""
    g = torch.Generator().manual_seed(5)
    for dtype, name, causal, groups, scale in ((torch.bfloat16, "bf16", True, 4, 8.0), (torch.float16, "f16", False, 1, 16.0)):
        q, k, v, do = (torch.randn((1, 1, n_, 32), generator=g).to(dtype) for n_ in (50, 70, 70, 50))
        mask = None if causal else (torch.rand((1, 70), generator=g) > 0.3)
        got = FR.grads_operand_faithful(q[0, 0], k[0, 0], v[0, 0], do[0, 0], None if mask is None else mask[0], causal, scale, groups, dtype)
        ref = O.attention_backward(_np(do), _np(q), _np(k), _np(v), mask=None if mask is None else mask.numpy(), scale=scale,
                                   groups=groups, causal=causal, operand_dtype=name, eps=1e-300)
        for a, r in zip(got, ref[:3]):
            assert np.abs(_np(a) - r[0, 0]).max() <= 1e-9 * max(1.0, np.abs(r).max())


def test_restated_rules_still_stand_in_their_sources():
    """the floors, the short-sequence factor, float32's zero-gradient allowance and the tangent bars that fullsize_reference.py restates are
    literals inside functions of three GPU test files: this fails when one of those files no longer carries them, so the copies cannot
    drift apart silently"""
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    for fn, literals in FR.RESTATED_FROM.items():
        src = open(os.path.join(here, fn)).read()
        for lit in literals:
            assert lit in src, (fn, lit)
    assert (FR.REL_FLOOR, FR.GRAD_FLOOR["f32"], FR.GRAD_FLOOR["bf16"], FR.F32_ZERO_GRAD_ABS, FR.SHORT_SEQUENCE_FACTOR, FR.SHORT_SEQUENCE_ROWS) == \
        (1e-3, 5e-2, 1e-3, 6e-6, 4.0, 100) and FR.TANGENT_BAR == {"bf16": 6e-2, "f16": 1.5e-2, "f32": 1.5e-2}


def test_round_to_float16_is_numpys_single_rounding():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(200000, generator=g, dtype=torch.float64) * 3
    p2 = torch.exp2(torch.randint(-16, 15, (50000,), generator=g).double())
    below = p2 * (1 - 2.0 ** -12) * (1 + torch.rand(50000, generator=g, dtype=torch.float64) * 2.0 ** -26)      # just above the tie under a power of two
    x = torch.cat([x, x * 1e-4, x * 1e-6, below, -below, torch.tensor([0.0, 65504.0, 1.0, 2.0 ** -14, 1.5 * 2.0 ** -24], dtype=torch.float64)])
    assert np.array_equal(FR.round_to(x, torch.float16).numpy(), x.numpy().astype(np.float16).astype(np.float64))


# ---- the probes ---------------------------------------------------------------------------------------------------------------------------

# N, M, window, causal: both sides bounded, one side open, N != M both ways (rows without a visible key), a window wider than a tile
PROBE_SHAPES = [(300, 300, (70, 0), True), (257, 400, (129, 33), False), (400, 257, (64, -1), False), (520, 520, (-1, 0), True), (130, 700, (300, 300), False)]


def _dense_probe(dtype, B, H, Hk, N, M, D):
    u = FR.unit_vector(D, FR.DT[dtype])
    q, k = u.expand(B, H, N, D).contiguous(), u.expand(B, Hk, M, D).contiguous()
    v, pos = FR.probe_v(list(range(B * Hk)), M, D, FR.DT[dtype])
    return q, k, v.view(B, Hk, M, D), pos.view(B, Hk, D)


@pytest.mark.parametrize("N,M,window,causal", PROBE_SHAPES)
def test_probe_closed_forms_equal_the_numpy_oracle(N, M, window, causal):
    D, G = 32, 2
    q, k, v, pos = _dense_probe("f32", 1, G, 1, N, M, D)
    do = torch.randn(1, G, N, D, generator=torch.Generator().manual_seed(N + M), dtype=torch.float64)
    okw = dict(causal=causal, attn_bias=np.repeat(band(N, M, *window, causal), G, axis=0), eps=1e-300)
    nk, nv = (np.repeat(_np(t), G, axis=1) for t in (k, v))
    ro, _ = O.attention_forward_stats(_np(q), nk, nv, **okw)
    _, _, rdv, _ = O.attention_backward(_np(do), _np(q), nk, nv, **okw)
    eo = FR.probe_expected_o(N, M, window, causal, pos[0, 0])
    assert np.abs(_np(eo)[None] - ro[0]).max() <= 1e-9 * max(1.0, np.abs(ro).max())
    edv = FR.probe_expected_dv(do[0], M, window, causal)
    assert np.abs(_np(edv) - rdv[0].sum(0)).max() <= 1e-9 * max(1.0, np.abs(rdv).max())
    assert pos[0, 0, 0] == 0 and pos[0, 0, 1] == M - 1          # the first and the last key carry a sentinel


@pytest.mark.parametrize("N,M,window,causal", PROBE_SHAPES + [(40, 40, (0, 0), False), (60, 30, (1, 0), True), (1, 1, (-1, -1), True), (5, 1, (-1, -1), False)])
def test_zero_gradient_rows_are_the_rows_the_oracle_gives_no_gradient(N, M, window, causal):
    """the rows the tangent-space identity of test_gpu_fullsize_features.py leaves out: dq / dk exactly 0 in the float64 oracle there, and
    nowhere else on random data"""
    g = torch.Generator().manual_seed(N * M)
    q, k, v, do = (torch.randn(1, 1, n_, 16, generator=g, dtype=torch.float64) for n_ in (N, M, M, N))
    rdq, rdk, _, _ = O.attention_backward(_np(do), _np(q), _np(k), _np(v), causal=causal, attn_bias=band(N, M, *window, causal), eps=1e-300)
    q_zero, k_zero = FR.zero_gradient_rows(N, M, window, causal)
    # (the oracle's P = P~ / l is 1 to an ulp there, so "zero" is its float64 residue: 1e-16 against gradients of 1e-2 ... 3 elsewhere)
    for ref, zero in ((rdq, q_zero), (rdk, k_zero)):
        size = np.abs(ref[0, 0]).max(-1)
        assert (size[zero.numpy()] <= 1e-12).all() and (size[~zero.numpy()] >= 1e-6).all()


def test_sentinels_cover_the_edges_they_promise():
    """over the units of a case: first and last key, every residue next to a 64- / 128- / 256-key tile edge, and for each sentinel away
    from the ends both rows next to each bounded band edge exist (so the whole-tensor comparison is an off-by-one test of both edges)"""
    L, D = 4096, 64
    pos = torch.stack([FR.sentinel_positions(u, L, D) for u in range(8)])
    assert (pos[:, 0] == 0).all() and (pos[:, 1] == L - 1).all()
    assert {int(p) % 256 for p in pos[:, 2:].flatten()} == set(FR.EDGE_RESIDUES)
    assert len({int(p) // 256 for p in pos.flatten()}) == L // 256          # every 256-key tile holds a sentinel
    left = 1024
    lo, hi, _ = FR.visible_range(L, L, (left, 0), True)
    for p in pos.flatten().tolist():
        if 0 < p < L - left - 1:
            assert lo[p + left] == p and lo[p + left + 1] == p + 1 and hi[p] == p and hi[p - 1] == p - 1


def _judge(label, dtype, got, expected):
    pattern, rel = FR.probe_compare(got, expected)
    print(f"{label}: zero pattern {'exact' if pattern else 'WRONG'}, worst relative error {rel:.3e} (bar {T.FWD_TOL[dtype][1]:.3e})")
    return pattern and T.check("probe/cpu-path/" + label, dtype, rel, T.FWD_TOL[dtype][1], label)


def _dense_expected(pos, H, N, M, window, causal):
    B, Hk, _ = pos.shape
    return torch.stack([torch.stack([FR.probe_expected_o(N, M, window, causal, pos[b, h // (H // Hk)]) for h in range(H)]) for b in range(B)])


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("N,M,window,causal", PROBE_SHAPES[:4])
def test_probe_forward_on_the_cpu_path_dense_window(dtype, N, M, window, causal):
    import flash_cosine_sim_attention_amd as F
    B, H, Hk, D = 2, 4, 2, 64
    q, k, v, pos = _dense_probe(dtype, B, H, Hk, N, M, D)
    o = F.flash_cosine_sim_attention_local(q, k, v, window, causal=causal)
    assert _judge(f"dense {dtype} n{N} m{M} {window}", dtype, o, _dense_expected(pos, H, N, M, window, causal))


PACKED_LQ, PACKED_LK = [300, 0, 1, 129, 257, 64], [300, 5, 1, 200, 257, 0]


def _packed_probe(dtype, lq, lk, H, Hk, D):
    u = FR.unit_vector(D, FR.DT[dtype])
    q, k = u.expand(sum(lq), H, D).contiguous(), u.expand(sum(lk), Hk, D).contiguous()
    v = torch.cat([FR.probe_v([s * Hk + h for h in range(Hk)], L, D, FR.DT[dtype])[0].permute(1, 0, 2) for s, L in enumerate(lk)])
    return q, k, v


def _packed_expected(v, cq, ck, H, window, causal):
    """closed form of a packed probe from v AS THIS SIDE SLICES IT by the offsets cq / ck"""
    Hk = v.shape[1]
    out = torch.zeros((cq[-1], H, v.shape[2]), dtype=torch.float64)
    for s in range(len(cq) - 1):
        vseq = v[ck[s]:ck[s + 1]].permute(1, 0, 2)
        out[cq[s]:cq[s + 1]] = FR.probe_expected_sequence(vseq, cq[s + 1] - cq[s], window, causal, H // Hk).permute(1, 0, 2)
    return out


def _packed_call(dtype, window, causal):
    import flash_cosine_sim_attention_amd as F
    H, Hk, D = 4, 2, 64
    q, k, v = _packed_probe(dtype, PACKED_LQ, PACKED_LK, H, Hk, D)
    cq, ck = np.concatenate([[0], np.cumsum(PACKED_LQ)]).tolist(), np.concatenate([[0], np.cumsum(PACKED_LK)]).tolist()
    o = F.flash_cosine_sim_attention_varlen(q, k, v, torch.tensor(cq, dtype=torch.int32), torch.tensor(ck, dtype=torch.int32), causal=causal,
                                            window_size=window)
    return o, v, cq, ck, H


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("window,causal", [((70, 0), True), ((-1, -1), False), ((100, 20), False)])
def test_probe_forward_on_the_cpu_path_packed(dtype, window, causal):
    o, v, cq, ck, H = _packed_call(dtype, window, causal)
    assert _judge(f"packed {dtype} {window}", dtype, o, _packed_expected(v, cq, ck, H, window, causal))


def _decode_probe(dtype, B, H, Hk, N, D, page, nb_seq, lens, n_new, seed=0):
    """a paged (page > 0) or contiguous decode probe: every sequence's logical V holds its sentinels over the L_b positions after the
    append; the first lens[b] of them sit in the cache, the rest arrive as v_new.  Cache positions beyond a sequence's length and pool
    blocks outside the table hold NaN.  Returns q, k_cache, v_cache, k_new, v_new, table, logical V per sequence."""
    dt = FR.DT[dtype]
    u = FR.unit_vector(D, dt)
    cap = nb_seq * page if page else nb_seq
    q = u.expand(B, H, N, D).contiguous()
    table = None
    if page:
        spare = 3
        perm = torch.randperm(B * nb_seq + spare, generator=torch.Generator().manual_seed(seed))
        table = perm[:B * nb_seq].to(torch.int32).view(B, nb_seq)
        kc = torch.full((B * nb_seq + spare, Hk, page, D), float("nan"), dtype=dt)
    else:
        kc = torch.full((B, Hk, cap, D), float("nan"), dtype=dt)
    vc = kc.clone()
    logical = []
    for b, n0 in enumerate(lens):
        L = min(n0 + n_new, cap)
        vl = FR.probe_v([b * Hk + h for h in range(Hk)], L, D, dt)[0]          # [Hk, L, D]
        logical.append(vl)
        for p in range(n0):
            if page:
                kc[int(table[b, p // page]), :, p % page], vc[int(table[b, p // page]), :, p % page] = u, vl[:, p]
            else:
                kc[b, :, p], vc[b, :, p] = u, vl[:, p]
    kn = vn = None
    if n_new:
        kn = u.expand(B, Hk, n_new, D).contiguous()
        vn = torch.zeros(B, Hk, n_new, D, dtype=dt)
        for b, n0 in enumerate(lens):
            L = logical[b].shape[1]
            vn[b, :, :L - n0] = logical[b][:, n0:L]
    return q, kc, vc, kn, vn, table, logical


def _decode_expected(vc, table, after, N, H, window, causal):
    Hk = vc.shape[1]
    return torch.stack([FR.probe_expected_sequence(FR.sequence_of_cache(vc, b, L, table), N, window, causal, H // Hk) for b, L in enumerate(after)])


def _decode_call(dtype, page, window, causal, N=5, n_new=5):
    import flash_cosine_sim_attention_amd as F
    B, H, Hk, D = 3, 4, 2, 32
    lens = [300, 0, 59]          # (59 + 5 crosses the edge of a 16- / 64-position page)
    q, kc, vc, kn, vn, table, _ = _decode_probe(dtype, B, H, Hk, N, D, page, (320 // page) if page else 320, lens, n_new)
    with torch.no_grad():
        o = F.flash_cosine_sim_attention_with_kvcache(q, kc, vc, kn, vn, cache_seqlens=torch.tensor(lens, dtype=torch.int32), block_table=table,
                                                      causal=causal, window_size=window)
    return o, vc, table, [n + n_new for n in lens], N, H


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("page,window,causal", [(0, (70, 0), True), (16, (-1, -1), True), (64, (100, 2), False), (16, (40, 0), True)])
def test_probe_forward_on_the_cpu_path_kvcache(dtype, page, window, causal):
    o, vc, table, after, N, H = _decode_call(dtype, page, window, causal)
    assert _judge(f"decode {dtype} page {page} {window}", dtype, o, _decode_expected(vc, table, after, N, H, window, causal))


# ---- discriminating power: a mistake on the expectation side is noticed ---------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_probe_notices_a_left_edge_off_by_one(dtype):
    import flash_cosine_sim_attention_amd as F
    N, M, window, causal = PROBE_SHAPES[0]
    q, k, v, pos = _dense_probe(dtype, 2, 4, 2, N, M, 64)
    o = F.flash_cosine_sim_attention_local(q, k, v, window, causal=causal)
    assert _judge("dense", dtype, o, _dense_expected(pos, 4, N, M, window, causal))
    for wrong in ((window[0] + 1, window[1]), (window[0] - 1, window[1])):
        assert not _judge("dense, left off by one", dtype, o, _dense_expected(pos, 4, N, M, wrong, causal))
    # the same through the float64 slice reference on random data: one key of 71 moves an output by far more than the oracle-pin bar
    g = torch.Generator().manual_seed(1)
    qr, kr, vr = torch.randn(2, N, 64, generator=g), torch.randn(M, 64, generator=g), torch.randn(M, 64, generator=g)
    a, b = FR.attention_slice(qr, kr, vr, causal=True, window=window), FR.attention_slice(qr, kr, vr, causal=True, window=(window[0] + 1, 0))
    assert (a - b).abs().max() > 1e-4


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_probe_notices_two_swapped_block_table_entries(dtype):
    o, vc, table, after, N, H = _decode_call(dtype, 16, (-1, -1), True)
    assert _judge("decode", dtype, o, _decode_expected(vc, table, after, N, H, (-1, -1), True))
    # (a swap is seen where one of the two pages holds a sentinel: here the pages of sequence 0's first and last key)
    wrong = table.clone()
    wrong[0, 0], wrong[0, 19] = table[0, 19], table[0, 0]
    assert not _judge("decode, table entries swapped", dtype, o, _decode_expected(vc, wrong, after, N, H, (-1, -1), True))


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_probe_notices_a_packed_offset_off_by_one_row(dtype):
    o, v, cq, ck, H = _packed_call(dtype, (70, 0), True)
    assert _judge("packed", dtype, o, _packed_expected(v, cq, ck, H, (70, 0), True))
    wrong = list(ck)
    wrong[4] += 1          # the key span of sequence 4 starts (and sequence 3 ends) one row late
    assert not _judge("packed, key offset off by one", dtype, o, _packed_expected(v, cq, wrong, H, (70, 0), True))
    wrong = list(cq)
    wrong[3] -= 1          # the query span of sequence 3 starts one row early (in sequence 2's only row)
    assert not _judge("packed, query offset off by one", dtype, o, _packed_expected(v, wrong, ck, H, (70, 0), True))
