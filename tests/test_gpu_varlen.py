"""Packed variable-length sequences on the GPU (flash_cosine_sim_attention_varlen, fcsa_forward_varlen / fcsa_backward_varlen).

The contract: each sequence's rows are what the dense op returns for that sequence alone as a [1, H, N_s, D] problem.  The reference is
the float64 oracle run per sequence (K/V repeated over each group for grouped-query heads, dk / dv summed back); sequences with an empty
query or key span have o = 0, dq = 0 (no key) and dk = dv = 0 (no query).  Equal-length sequences on shapes where the dense dispatch takes
no split, 64-rows-per-wave or group-sweep form must match the dense [S, H, L, D] call bit for bit (same form, same grid); a NaN-filled
arena with guard bands checks that the packed calls stay inside their buffers and write every output row."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases as GC
import tolerances as T
import varlen_form_cases as VF
from oracle import cosine_sim_oracle as O

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def _np(t):
    return t.detach().cpu().double().numpy()


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-3 * np.sqrt(max(b.size, 1))))


def _cu(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)


def _packed_inputs(dtype, lq, lk, H, Hk, D, seed, l2norm=True):
    dt = DT[dtype]
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32)
    TQ, TK = int(sum(lq)), int(sum(lk))
    q, k, v, do = rnd(TQ, H, D), rnd(TK, Hk, D), rnd(TK, Hk, D), rnd(TQ, H, D)
    if not l2norm:
        q, k = torch.nn.functional.normalize(q, dim=-1), torch.nn.functional.normalize(k, dim=-1)
    return tuple(t.to(dt) for t in (q, k, v, do))


def _oracle(q, k, v, do, lq, lk, H, Hk, kw):
    """Per-sequence float64 reference of (o, dq, dk, dv), packed like the inputs.  In the per-row-shift regime (logit range beyond the
    static exponent window) the 16-bit cases are compared with exact math on the 16-bit operands, as in test_gpu_parity.py: the rounding of
    c1 * q^ alone moves a logit of range +-100 by more than the raw-input bars allow."""
    dyn = kw.get("scale", 8.0) * kw.get("groups", 1) > 11
    opd = {torch.float16: "f16", torch.bfloat16: "bf16"}.get(q.dtype) if dyn else None
    G = H // Hk
    ro, rdq = np.zeros(q.shape), np.zeros(q.shape)
    rdk, rdv = np.zeros(k.shape), np.zeros(k.shape)
    nq, nk, nv, ndo = _np(q), _np(k), _np(v), _np(do)
    cq, ck = np.concatenate([[0], np.cumsum(lq)]), np.concatenate([[0], np.cumsum(lk)])
    for s in range(len(lq)):
        if lq[s] == 0 or lk[s] == 0:
            continue
        sq, sk = slice(cq[s], cq[s + 1]), slice(ck[s], ck[s + 1])
        qs, dos = nq[sq].transpose(1, 0, 2)[None], ndo[sq].transpose(1, 0, 2)[None]
        ks, vs = (np.repeat(x[sk].transpose(1, 0, 2)[None], G, axis=1) for x in (nk, nv))
        # (the per-row-shift regime normalises rows exactly: no 1e-10 clamp in the reference there, as in test_gpu_parity.py)
        okw = dict(kw, eps=1e-300 if dyn else 1e-10, operand_dtype=opd)
        o, _ = O.attention_forward_stats(qs, ks, vs, **okw)
        dq, dk, dv, _ = O.attention_backward(dos, qs, ks, vs, **okw)
        ro[sq] = o[0].transpose(1, 0, 2)
        rdq[sq] = dq[0].transpose(1, 0, 2)
        rdk[sk] = dk[0].reshape(Hk, G, lk[s], -1).sum(1).transpose(1, 0, 2)
        rdv[sk] = dv[0].reshape(Hk, G, lk[s], -1).sum(1).transpose(1, 0, 2)
    return ro, rdq, rdk, rdv


def _run(q, k, v, do, lq, lk, kw, max_q=None, max_k=None):
    import flash_cosine_sim_attention_amd as F
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    o = F.flash_cosine_sim_attention_varlen(q, k, v, _cu(lq), _cu(lk), max_seqlen_q=max_q, max_seqlen_k=max_k, **kw)
    o.backward(do)
    torch.cuda.synchronize()
    return o.detach(), q.grad, k.grad, v.grad


def _check(dtype, got, ref, lq, lk, label, atol_scale=1.0, excess_ref=None):
    """excess_ref: the reference of the elementwise forward check where it is not ref's o (see test_varlen_forms)"""
    o, dq, dk, dv = got
    ro, rdq, rdk, rdv = ref
    atol, rtol, rel = T.FWD_TOL[dtype]
    atol *= atol_scale
    go = _np(o)
    for nm, g in zip(("o", "dq", "dk", "dv"), (o, dq, dk, dv)):
        assert torch.isfinite(g).all(), (label, nm)
    re = ro if excess_ref is None else excess_ref
    assert T.check(label + "/fwd-excess", dtype, float((np.abs(go - re) - rtol * np.abs(re)).max(initial=0.0)), atol), label
    assert T.check(label + "/fwd-rel", dtype, _rel(go, ro), rel), label
    bar = T.GRAD_TOL[dtype] * T.SPLIT_GRAD_FACTOR[dtype]
    for nm, g, r in (("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
        assert T.check(f"{label}/{nm}", dtype, _rel(_np(g), r), bar), (label, nm, _rel(_np(g), r), bar)
    # per sequence: a row bound to the wrong span shows as an O(1) error in its own sequence, whatever the whole tensor's norm
    cq, ck = np.concatenate([[0], np.cumsum(lq)]), np.concatenate([[0], np.cumsum(lk)])
    for s in range(len(lq)):
        sq, sk = slice(cq[s], cq[s + 1]), slice(ck[s], ck[s + 1])
        if lk[s] == 0:
            assert (o[sq] == 0).all() and (dq[sq] == 0).all(), (label, s, "no key: o and dq must be zero")
        if lq[s] == 0:
            assert (dk[sk] == 0).all() and (dv[sk] == 0).all(), (label, s, "no query: dk and dv must be zero")
        if lq[s] and lk[s]:
            # (norms relative to the sequence's share of the whole tensor's: a one-query causal sequence has dq = 0 exactly, and the
            #  kernels' rounding residue there is no error of the span)
            for nm, g, r, sl in (("o", o, ro, sq), ("dq", dq, rdq, sq), ("dk", dk, rdk, sk), ("dv", dv, rdv, sk)):
                floor = np.linalg.norm(r) * np.sqrt(r[sl].size / r.size)
                err = np.linalg.norm(_np(g)[sl] - r[sl]) / max(np.linalg.norm(r[sl]), floor, 1e-30)
                assert err <= 4 * (rel if nm == "o" else bar), (label, s, nm, err)


# id, dtype, query lengths, key lengths (None: the query lengths), H, Hk, D, kwargs
EDGE = [0, 1, 127, 128, 129, 300]
CASES = [
    ("bf16_d64_causal_edges", "bf16", EDGE, None, 4, 4, 64, dict(causal=True)),
    ("f16_d64_edges", "f16", EDGE, None, 4, 4, 64, dict()),
    ("f32_d64_causal_edges", "f32", EDGE, None, 2, 2, 64, dict(causal=True)),
    ("bf16_d16_causal_n_gt_m", "bf16", [200, 130, 1, 64], [150, 129, 3, 0], 4, 4, 16, dict(causal=True)),
    ("f16_d32_causal_n_lt_m", "f16", [100, 5, 0, 257], [190, 40, 7, 300], 4, 4, 32, dict(causal=True)),
    ("bf16_d96_noncausal_n_ne_m", "bf16", [129, 60, 301], [300, 61, 0], 2, 2, 96, dict()),
    ("f16_d128_causal_long", "f16", [1500, 7, 900], None, 2, 2, 128, dict(causal=True)),
    ("bf16_d128_noncausal", "bf16", [333, 1, 640], [700, 65, 2], 4, 4, 128, dict()),
    ("f32_d128_causal", "f32", [140, 0, 75], [140, 3, 90], 2, 2, 128, dict(causal=True)),
    ("f32_d16_noncausal", "f32", [60, 129], [200, 1], 2, 2, 16, dict()),
    ("f16_d96_causal", "f16", [257, 31], [257, 64], 2, 2, 96, dict(causal=True)),
    ("f32_d32_groups2", "f32", [100, 50], [120, 60], 2, 2, 32, dict(groups=2, scale=4.0)),
    ("bf16_d64_groups4", "bf16", [300, 129, 0], [260, 129, 5], 4, 4, 64, dict(groups=4, scale=2.0, causal=True)),
    ("bf16_d96_groups2_slabs", "bf16", [100, 150], [129, 90], 2, 2, 96, dict(groups=2, scale=4.0)),
    ("f16_d64_no_l2norm", "f16", [129, 300, 1], [257, 100, 0], 4, 4, 64, dict(l2norm_qk=False, scale=1.0)),
    ("bf16_d64_per_row_shift", "bf16", [200, 0, 333], [250, 9, 333], 4, 4, 64, dict(scale=100.0, causal=True)),
    ("f16_d64_per_row_shift_empty_keys", "f16", [150, 40], [0, 90], 2, 2, 64, dict(scale=16.0)),
    ("bf16_d64_gqa", "bf16", [300, 7, 129], [250, 7, 400], 8, 2, 64, dict(causal=True)),
    ("f16_d128_single_kv", "f16", [129, 200], [300, 1], 4, 1, 128, dict()),
    ("f32_d64_gqa_single", "f32", [77, 130], [90, 0], 4, 1, 64, dict(causal=True)),
]


@pytest.mark.parametrize("name,dtype,lq,lk,H,Hk,D,kw", CASES, ids=[c[0] for c in CASES])
def test_varlen_parity(name, dtype, lq, lk, H, Hk, D, kw):
    lk = lq if lk is None else lk
    q, k, v, do = _packed_inputs(dtype, lq, lk, H, Hk, D, seed=sum(map(ord, name)), l2norm=kw.get("l2norm_qk", True))
    got = _run(q, k, v, do, lq, lk, kw)
    _check(dtype, got, _oracle(q, k, v, do, lq, lk, H, Hk, kw), lq, lk, name)


@pytest.mark.parametrize("name,dtype,D,lq,lk,H,Hk,mx,kw", VF.CASES, ids=[c[0] for c in VF.CASES])
def test_varlen_forms(name, dtype, D, lq, lk, H, Hk, mx, kw):
    """every kernel form a packed call can reach (tests/varlen_form_cases.py; test_varlen_forms_cpu.py checks that the table launches them
    all): 8-wave 256-position tiles, lean, two-wave dQ, key / query split halves and 4-wave forms, on ragged spans"""
    q, k, v, do = _packed_inputs(dtype, lq, lk, H, Hk, D, seed=sum(map(ord, name)), l2norm=kw.get("l2norm_qk", True))
    got = _run(q, k, v, do, lq, lk, kw, max_q=mx, max_k=mx)
    l2, scale, groups = kw.get("l2norm_qk", True), kw.get("scale", 8.0), kw.get("groups", 1)
    atol_scale, excess_ref = 1.0, None
    if GC.dynamic_shift_regime(dtype, scale, groups, l2, False):
        if dtype == "f32":
            atol_scale = T.f32_per_row_excess_factor(scale, groups)
        else:
            excess_ref = _oracle_forward_kernel_k(q, k, v, lq, lk, H, Hk, kw, mx)
    _check(dtype, got, _oracle(q, k, v, do, lq, lk, H, Hk, kw), lq, lk, name, atol_scale, excess_ref)


def _oracle_forward_kernel_k(q, k, v, lq, lk, H, Hk, kw, mx):
    """16-bit, per-row shift: the operand-faithful forward reference (exact math on the 16-bit operands) with K^ as the kernel rounded it.
    The l2norm kernel normalises in float32; where an element of the float64 K^ lies within float32 error of a rounding midpoint, its
    16-bit K^ is the other neighbour than the oracle's.  At scale x groups = 80 one such element of a dominant key moves an output by
    up to 0.03 (bf16: 2.7e-2 excess against the 2e-2 bar, with the kernel's K^ 2e-5) -- a property of normalising before rounding, not
    of a form.  The saved K^ is checked here against the float64 one: equal after rounding except at a few midpoints, one ulp off."""
    from flash_cosine_sim_attention_amd import _torch_ops
    scale, groups, causal = kw.get("scale", 8.0), kw.get("groups", 1), kw.get("causal", False)
    opd = {torch.float16: "f16", torch.bfloat16: "bf16"}[q.dtype]
    kn = _torch_ops.load().varlen_forward(q, k, v, _cu(lq).cuda(), _cu(lk).cuda(), mx or max(lq), mx or max(lk), float(scale), bool(causal),
                                          True, int(groups), True)[3]
    kn = kn.double().cpu().numpy()                                      # [Hk, total_k, D]
    kh = O.l2norm(_np(k).transpose(1, 0, 2)[None], groups)[0]
    other = kn != O.round_to(kh, opd)
    # (midpoints within float32 error: ~1e-5 of the bf16 elements, ~1e-4 of the f16 ones, three more bits; measured 1.4e-4 at most)
    assert other.mean() <= (1e-4 if opd == "bf16" else 1e-3), ("saved K^ differs from the rounded float64 K^ in", int(other.sum()), "elements")
    one_ulp = 2.0 ** (-7 if opd == "bf16" else -10)
    assert (np.abs(kn - kh) <= one_ulp * np.abs(kh))[other].all(), "saved K^ more than one 16-bit step from the float64 K^"
    G = H // Hk
    ro = np.zeros(q.shape)
    nq, nv = _np(q), _np(v)
    cq, ck = np.concatenate([[0], np.cumsum(lq)]), np.concatenate([[0], np.cumsum(lk)])
    for s in range(len(lq)):
        if lq[s] == 0 or lk[s] == 0:
            continue
        sq, sk = slice(cq[s], cq[s + 1]), slice(ck[s], ck[s + 1])
        qh = O.l2norm(nq[sq].transpose(1, 0, 2)[None], groups)
        khs = np.repeat(kn[:, sk][None], G, axis=1)
        vs = np.repeat(nv[sk].transpose(1, 0, 2)[None], G, axis=1)
        o, _ = O.attention_forward_stats(qh, khs, vs, scale=scale, causal=causal, l2norm_qk=False, eps=1e-300, operand_dtype=opd)
        ro[sq] = o[0].transpose(1, 0, 2)
    return ro


def test_varlen_many_short_sequences_and_large_max_seqlen():
    rng = np.random.default_rng(5)
    lq = rng.integers(0, 40, size=520).tolist()
    lk = rng.integers(0, 40, size=520).tolist()
    q, k, v, do = _packed_inputs("bf16", lq, lk, 2, 2, 64, seed=11)
    kw = dict(causal=True)
    # max_seqlen well above every span: more idle workgroups, the same rows
    got = _run(q, k, v, do, lq, lk, kw, max_q=700, max_k=300)
    _check("bf16", got, _oracle(q, k, v, do, lq, lk, 2, 2, kw), lq, lk, "many_short")


def test_varlen_strided_views_of_one_packed_qkv():
    import flash_cosine_sim_attention_amd as F
    lq = [129, 64, 300, 1]
    H, D = 4, 64
    g = torch.Generator(device="cuda").manual_seed(3)
    qkv = torch.randn(sum(lq), 3, H, D, device="cuda", generator=g).to(torch.bfloat16)
    do = torch.randn(sum(lq), H, D, device="cuda", generator=g).to(torch.bfloat16)
    leaf = qkv.clone().requires_grad_()
    q, k, v = leaf[:, 0], leaf[:, 1], leaf[:, 2]
    assert not q.is_contiguous()
    o = F.flash_cosine_sim_attention_varlen(q, k, v, _cu(lq), _cu(lq), causal=True)
    o.backward(do)
    torch.cuda.synchronize()
    ref = _run(qkv[:, 0].contiguous(), qkv[:, 1].contiguous(), qkv[:, 2].contiguous(), do, lq, lq, dict(causal=True))
    assert torch.equal(o, ref[0])
    assert torch.equal(leaf.grad[:, 0], ref[1]) and torch.equal(leaf.grad[:, 1], ref[2]) and torch.equal(leaf.grad[:, 2], ref[3])


# equal-length sequences, shapes on which the dense dispatch takes no split, fwd2 / fwd3 or group sweep (grids that cover 256 CUs); then
# the 8-wave forms of varlen_form_cases.BIT_CASES
BIT_CASES = [
    ("bf16_d64_causal", "bf16", 8, 8, 1024, 64, True),
    ("f16_d64_noncausal", "f16", 4, 8, 1024, 64, False),
    ("bf16_d128_causal", "bf16", 8, 8, 1024, 128, True),
    ("bf16_d32_noncausal", "bf16", 4, 16, 512, 32, False),
] + VF.BIT_CASES


@pytest.mark.parametrize("name,dtype,S,H,L,D,causal", BIT_CASES, ids=[c[0] for c in BIT_CASES])
def test_varlen_equal_lengths_match_dense_bit_for_bit(name, dtype, S, H, L, D, causal):
    import flash_cosine_sim_attention_amd as F
    from flash_cosine_sim_attention_amd import _lib
    dt = DT[dtype]
    g = torch.Generator(device="cuda").manual_seed(7)
    q, k, v, do = (torch.randn(S, H, L, D, device="cuda", generator=g).to(dt) for _ in range(4))
    dense = [t.clone().requires_grad_() for t in (q, k, v)]
    # (D = 128: the dense call must not take the 64-rows-per-wave forward, which packed sequences never run)
    prev = _lib.forward_form(0) if D == 128 else None
    try:
        o = F.flash_cosine_sim_attention(*dense, causal=causal)
    finally:
        if prev is not None:
            _lib.forward_form(prev)
    o.backward(do)
    pack = lambda t: t.permute(0, 2, 1, 3).reshape(S * L, H, D)
    packed = [pack(t).clone().requires_grad_() for t in (q, k, v)]
    cu = _cu([L] * S)
    ov = F.flash_cosine_sim_attention_varlen(*packed, cu, cu, causal=causal)
    ov.backward(pack(do))
    torch.cuda.synchronize()
    assert torch.equal(ov, pack(o))
    for a, b in zip(packed, dense):
        assert torch.equal(a.grad, pack(b.grad))


def test_varlen_backward_is_deterministic():
    lq, lk = [300, 0, 129, 77], [250, 40, 129, 0]
    q, k, v, do = _packed_inputs("bf16", lq, lk, 8, 2, 64, seed=21)
    a = _run(q, k, v, do, lq, lk, dict(causal=True))
    b = _run(q, k, v, do, lq, lk, dict(causal=True))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- the C ABI on caller-owned buffers: a NaN-filled arena with guard bands (see test_gpu_buffer_bounds.py) ------------------------------
FILL, GUARD = 0xFF, 4096


class Arena:
    def __init__(self, nbytes):
        self.buf = torch.full((nbytes,), FILL, device="cuda", dtype=torch.uint8)
        self.off = GUARD
        self.used = []

    def take(self, shape, dtype):
        n = int(np.prod(shape))
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        off = (self.off + 255) // 256 * 256
        assert off + nbytes + GUARD <= self.buf.numel(), "arena too small"
        self.used.append((off, nbytes))
        self.off = off + nbytes + GUARD
        return self.buf[off:off + nbytes].view(dtype).view(shape)

    def guards_intact(self):
        keep = torch.ones(self.buf.numel(), device="cuda", dtype=torch.bool)
        for off, n in self.used:
            keep[off:off + n] = False
        return bool((self.buf[keep] == FILL).all().item())


BOUNDS = [
    ("bf16_d64_causal", "bf16", [129, 0, 300, 1, 64], [100, 7, 300, 0, 65], 4, 4, 64, dict(causal=True)),
    ("f16_d128_gqa", "f16", [257, 33], [140, 300], 4, 2, 128, dict()),
    ("f32_d96_groups2_single_kv", "f32", [70, 131], [131, 0], 2, 1, 96, dict(groups=2, scale=4.0)),
    ("bf16_d96_one_group", "bf16", [200, 3], [129, 9], 2, 2, 96, dict(causal=True)),
    ("f16_d64_per_row_shift", "f16", [150, 0, 40], [40, 20, 0], 2, 2, 64, dict(scale=16.0)),
] + VF.BOUNDS_CASES


@pytest.mark.parametrize("name,dtype,lq,lk,H,Hk,D,kw", BOUNDS, ids=[b[0] for b in BOUNDS])
def test_varlen_calls_stay_inside_their_buffers(name, dtype, lq, lk, H, Hk, D, kw):
    from flash_cosine_sim_attention_amd import _lib
    lib = _lib.load()
    dt = DT[dtype]
    causal, groups, scale = kw.get("causal", False), kw.get("groups", 1), kw.get("scale", 8.0)
    S, TQ, TK = len(lq), sum(lq), sum(lk)
    prob = _lib.problem(dt, (S, H, Hk, max(lq), max(lk), D), causal, False, True, groups, scale)
    es = torch.empty((), dtype=dt).element_size()
    ar0 = Arena(1 << 12)          # (tables first: their device copies live in their own arena)
    cuq, cuk = _cu(lq).cuda(), _cu(lk).cuda()
    seqs = _lib.Varlen(cuq.data_ptr(), cuk.data_ptr(), TQ, TK)
    bws_n = int(lib.fcsa_backward_varlen_workspace_bytes(C.byref(prob), C.byref(seqs)))
    total = (6 * TQ * H * D + 7 * TK * Hk * D) * es + (TQ * H * (1 + groups) + TK * Hk * groups) * 4 + bws_n + 40 * (GUARD + 256)
    ar = Arena(total)
    g = torch.Generator(device="cuda").manual_seed(sum(map(ord, name)))

    def rnd(shape):
        t = ar.take(shape, dt)
        t.copy_(torch.randn(shape, device="cuda", dtype=torch.float32, generator=g).to(dt))
        return t

    q, k, v, do = rnd((TQ, H, D)), rnd((TK, Hk, D)), rnd((TK, Hk, D)), rnd((TQ, H, D))
    inputs = (q, k, v, do, cuq, cuk)
    before = [t.clone() for t in inputs]
    o = ar.take((TQ, H, D), dt)
    inv_l = ar.take((H, TQ), torch.float32)
    qn, kn = ar.take((H, TQ, D), dt), ar.take((Hk, TK, D), dt)
    rq, rk = ar.take((H, TQ, groups), torch.float32), ar.take((Hk, TK, groups), torch.float32)
    dq, dk, dv = ar.take((TQ, H, D), dt), ar.take((TK, Hk, D), dt), ar.take((TK, Hk, D), dt)
    bws = ar.take((max(bws_n, 1),), torch.uint8)
    t3 = lambda t: _lib.Tensor(t.data_ptr(), 0, t.stride(1), t.stride(0))
    ptr = lambda t: t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    norm = _lib.NormState(ptr(qn), ptr(kn), ptr(rq), ptr(rk))
    fa = _lib.ForwardArgs(prob, t3(q), t3(k), t3(v), t3(o), ptr(inv_l), None, None, norm, None, 0, stream)
    _lib.check(lib.fcsa_forward_varlen(C.byref(fa), C.byref(seqs)), "fcsa_forward_varlen")
    ba = _lib.BackwardArgs(prob, t3(do), t3(o), ptr(inv_l), t3(q), t3(k), t3(v), None, None, norm, t3(dq), t3(dk), t3(dv), None,
                           ptr(bws), bws_n, stream)
    _lib.check(lib.fcsa_backward_varlen(C.byref(ba), C.byref(seqs)), "fcsa_backward_varlen")
    torch.cuda.synchronize()
    assert ar.guards_intact() and ar0.guards_intact()
    for a, b in zip(inputs, before):
        assert torch.equal(a, b)
    for nm, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert not torch.isnan(t).any(), (nm, "an output row was never written")


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
def test_varlen_opcheck():
    from flash_cosine_sim_attention_amd import _torch_ops
    fc = _torch_ops.load()
    lq, lk = [40, 0, 70], [50, 3, 70]
    q, k, v, do = _packed_inputs("bf16", lq, lk, 2, 2, 64, seed=2)
    cuq, cuk = _cu(lq).cuda(), _cu(lk).cuda()
    args = (q, k, v, cuq, cuk, 70, 70, 8.0, True, True, 1)
    torch.library.opcheck(fc.varlen_forward, args + (True,))
    o, inv_l, qn, kn, rq, rk = fc.varlen_forward(*args, True)
    torch.library.opcheck(fc.varlen_backward, (do, o, inv_l, q, k, v, cuq, cuk, qn, kn, rq, rk, 70, 70, 8.0, True, True, 1))
    torch.library.opcheck(fc.varlen_attention, (q.requires_grad_(), k.requires_grad_(), v.requires_grad_()) + args[3:])


def test_varlen_grad_scaler_training_step():
    import flash_cosine_sim_attention_amd as F
    torch.manual_seed(0)
    lens = [100, 37, 260]
    H, D = 4, 64
    proj = torch.nn.Linear(D, 3 * H * D, device="cuda")
    opt = torch.optim.SGD(proj.parameters(), lr=1e-2)
    scaler = torch.amp.GradScaler("cuda")
    x = torch.randn(sum(lens), D, device="cuda")
    cu = _cu(lens)
    with torch.autocast("cuda", dtype=torch.float16):
        qkv = proj(x).view(-1, 3, H, D)
        o = F.flash_cosine_sim_attention_varlen(qkv[:, 0], qkv[:, 1], qkv[:, 2], cu, cu, causal=True)
        loss = o.float().pow(2).mean()
    scaler.scale(loss).backward()
    scaler.step(opt)
    scaler.update()
    assert all(torch.isfinite(p.grad).all() for p in proj.parameters())
    assert proj.weight.grad.abs().sum() > 0


@pytest.mark.parametrize("cu,err", [
    ([1, 5, 9], "start at 0"),
    ([0, 10, 9], "non-decreasing"),
    ([0, 4, 8], "end at the packed length"),
])
def test_varlen_host_tables_are_validated_before_any_launch(cu, err):
    import flash_cosine_sim_attention_amd as F
    q = torch.randn(9, 2, 64, device="cuda", dtype=torch.bfloat16)
    good = _cu([4, 5])
    bad = torch.tensor(cu, dtype=torch.int32)
    with pytest.raises(ValueError, match=err):
        F.flash_cosine_sim_attention_varlen(q, q, q, bad, good)
    with pytest.raises(ValueError, match="longer than max_seqlen"):
        F.flash_cosine_sim_attention_varlen(q, q, q, good, good, max_seqlen_q=4)
