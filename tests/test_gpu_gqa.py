"""Grouped-query attention on the GPU: k, v of shape [B, Hk, M, D] with 1 < Hk < H and H % Hk == 0; query head h attends to K/V head
h // (H // Hk).  The reference result is the float64 oracle run on K/V repeated to H heads (np.repeat over the head axis); the reference
dk / dv are the oracle's per-query-head gradients summed over each group.  Both dK/dV forms are pinned with the C ABI knob
(fcsa_debug_kv_group_form): 0 = per-query-head f32 slabs + finalize, 2 = the in-kernel group sweep wherever it is compiled (16-bit,
bias-free, D = 64 / 128; every other case takes the slab route under both settings).  The slab sums and the sweep's register sums are
both f32 sums over the group, so the gradient bars carry SPLIT_GRAD_FACTOR."""
import ctypes as C
import contextlib

import numpy as np
import pytest
import torch

import tolerances as T
from oracle import cosine_sim_oracle as O

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


@contextlib.contextmanager
def kv_form(form):
    from flash_cosine_sim_attention_amd import _lib
    prev = _lib.kv_group_form(form)
    try:
        yield
    finally:
        _lib.kv_group_form(prev)


def _np(t):
    return None if t is None else (t.detach().cpu().double().numpy() if t.is_floating_point() else t.detach().cpu().numpy())


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-3 * np.sqrt(b.size)))


# id, dtype, B, H, Hk, N, M, D, kwargs
CASES = [
    ("bf16_d64_g4_causal_n_ne_m", "bf16", 2, 8, 2, 200, 260, 64, dict(causal=True)),
    ("f16_d64_g2_mask", "f16", 2, 4, 2, 130, 300, 64, dict(mask=True)),
    ("bf16_d128_g3_causal", "bf16", 1, 6, 2, 257, 300, 128, dict(causal=True)),
    ("f16_d128_g8_single_kv_control", "f16", 1, 8, 1, 77, 129, 128, dict()),      # Hk = 1: single-headed K/V, through the same checks
    ("f16_d128_g8", "f16", 1, 16, 2, 77, 129, 128, dict()),
    ("bf16_d16_g2_causal", "bf16", 2, 4, 2, 150, 150, 16, dict(causal=True)),
    ("f16_d32_g4_groups4", "f16", 1, 8, 2, 100, 190, 32, dict(groups=4, scale=2.0)),      # (logit range scale * groups inside f16's static window)
    ("bf16_d96_g2", "bf16", 1, 4, 2, 140, 170, 96, dict()),
    ("f32_d64_g2_causal", "f32", 1, 4, 2, 100, 150, 64, dict(causal=True)),
    ("f32_d128_g3_mask", "f32", 1, 6, 2, 70, 131, 128, dict(mask=True)),
    ("bf16_d64_g2_bias_head", "bf16", 1, 4, 2, 100, 140, 64, dict(bias=True)),
    ("f16_d64_g4_bias_batch", "f16", 2, 8, 2, 90, 120, 64, dict(bias=True, bias_batch=True, scale=4.0)),
    ("bf16_d64_g2_groups8", "bf16", 1, 4, 2, 160, 160, 64, dict(groups=8, scale=2.0)),
    ("f16_d128_g2_no_l2norm", "f16", 1, 4, 2, 129, 257, 128, dict(l2norm=False, scale=1.0)),
    ("bf16_d64_g2_no_l2norm_causal", "bf16", 2, 4, 2, 100, 100, 64, dict(l2norm=False, scale=1.0, causal=True)),
    ("bf16_d64_g2_split_queries", "bf16", 1, 4, 2, 3000, 200, 64, dict()),      # split-query dK/dV slabs: [B][H x splits][M][D]
    ("f16_d128_g4_small_grid_causal", "f16", 1, 8, 2, 1100, 1100, 128, dict(causal=True)),
    ("bf16_d64_g2_strided_kv", "bf16", 2, 4, 2, 120, 180, 64, dict(strided=True)),
    ("bf16_d96_g2_groups2_slabs", "bf16", 1, 4, 2, 100, 129, 96, dict(groups=2, scale=4.0)),     # l2norm groups the finalize kernel handles
]


def _inputs(dtype, B, H, Hk, N, M, D, kw, seed):
    dt = DT[dtype]
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32).to(dt)
    q, do = rnd(B, H, N, D), rnd(B, H, N, D)
    if kw.get("strided"):          # views into wider storage: head-major, padded rows
        k = rnd(Hk, B, M, D + 16).permute(1, 0, 2, 3)[..., 8:8 + D]
        v = rnd(Hk, B, M, D + 16).permute(1, 0, 2, 3)[..., :D]
    else:
        k, v = rnd(B, Hk, M, D), rnd(B, Hk, M, D)
    if not kw.get("l2norm", True):
        q = torch.nn.functional.normalize(q.float(), dim=-1).to(dt)
        k = torch.nn.functional.normalize(k.float(), dim=-1).to(dt)
    mask = None
    if kw.get("mask"):
        mask = torch.rand(B, M, device="cuda", generator=g) > 0.3
        mask[:, 0] = True
    bias = None
    if kw.get("bias"):
        bias = (0.5 * torch.randn((B if kw.get("bias_batch") else H), N, M, device="cuda", generator=g)).to(dt)
    return q, k, v, do, mask, bias


def _op_kw(kw):
    return dict(causal=kw.get("causal", False), groups=kw.get("groups", 1), scale=kw.get("scale", 8.0),
                l2norm_qk=kw.get("l2norm", True), attn_bias_batch_dim=kw.get("bias_batch", False))


def _run(q, k, v, do, mask, bias, kw, grads=True):
    import flash_cosine_sim_attention_amd as F
    q, k, v = (t.detach().clone().requires_grad_(grads) if not kw.get("strided") or t is q else t.detach().requires_grad_(grads)
               for t in (q, k, v))
    b = bias.detach().clone().requires_grad_(grads) if bias is not None else None
    o = F.flash_cosine_sim_attention(q, k, v, mask=mask, attn_bias=b, **_op_kw(kw))
    if not grads:
        torch.cuda.synchronize()
        return o.detach(), None, None, None, None
    o.backward(do)
    torch.cuda.synchronize()
    return o.detach(), q.grad, k.grad, v.grad, (b.grad if b is not None else None)


def _oracle(q, k, v, do, mask, bias, kw, H, Hk):
    G = H // Hk
    nq, nk, nv, ndo = _np(q), np.repeat(_np(k), G, axis=1), np.repeat(_np(v), G, axis=1), _np(do)
    okw = dict(mask=_np(mask), attn_bias=_np(bias), **_op_kw(kw))
    ro, _ = O.attention_forward_stats(nq, nk, nv, **okw)
    rdq, rdk, rdv, rdb = O.attention_backward(ndo, nq, nk, nv, **okw)
    B, _, M, D = rdk.shape
    return ro, rdq, rdk.reshape(B, Hk, G, M, D).sum(2), rdv.reshape(B, Hk, G, M, D).sum(2), rdb


def _check_forward(dtype, o, ro, label):
    atol, rtol, rel = T.FWD_TOL[dtype]
    got = _np(o)
    assert np.isfinite(got).all()
    assert T.check(label + "/fwd-excess", dtype, float((np.abs(got - ro) - rtol * np.abs(ro)).max()), atol), label
    assert T.check(label + "/fwd-rel", dtype, _rel(got, ro), rel), label


def _check_grads(dtype, got, ref, label):
    bar = T.GRAD_TOL[dtype] * T.SPLIT_GRAD_FACTOR[dtype]
    for nm, g, r in zip(("dq", "dk", "dv", "d_bias"), got, ref):
        if r is None:
            continue
        assert g is not None, nm
        assert tuple(g.shape) == r.shape, (nm, g.shape, r.shape)
        b = bar * (1.5 if nm == "d_bias" else 1.0)
        assert T.check(f"{label}/{nm}", dtype, _rel(_np(g), r), b), (nm, _rel(_np(g), r), b)


@pytest.mark.parametrize("name,dtype,B,H,Hk,N,M,D,kw", CASES, ids=[c[0] for c in CASES])
def test_gqa_parity_both_backward_forms(name, dtype, B, H, Hk, N, M, D, kw):
    q, k, v, do, mask, bias = _inputs(dtype, B, H, Hk, N, M, D, kw, seed=abs(hash(name)) % 10000)
    ro, rdq, rdk, rdv, rdb = _oracle(q, k, v, do, mask, bias, kw, H, Hk)
    res = {}
    for form in (0, 2):
        with kv_form(form):
            o, dq, dk, dv, db = _run(q, k, v, do, mask, bias, kw)
        assert o.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape
        _check_forward(dtype, o, ro, f"gqa/{name}/form{form}")
        _check_grads(dtype, (dq, dk, dv, db), (rdq, rdk, rdv, rdb if bias is not None else None), f"gqa/{name}/form{form}")
        res[form] = (o, dq, dk, dv)
    # the forward does not depend on the backward form; the two backward forms agree within the gradient bar
    assert torch.equal(res[0][0], res[2][0])
    assert torch.equal(res[0][1], res[2][1])          # dq: the same dQ kernel either way
    bar = T.GRAD_TOL[dtype] * T.SPLIT_GRAD_FACTOR[dtype]
    for i, nm in ((2, "dk"), (3, "dv")):
        assert T.check(f"gqa/{name}/forms-agree/{nm}", dtype, _rel(_np(res[2][i]), _np(res[0][i])), bar), nm


FWD_EQ = [
    # the GQA forward reads K/V head h // G where the expanded call reads head h of the repeated copy: the same bytes, the same kernel
    ("bf16_d64_causal", "bf16", 2, 8, 2, 300, 300, 64, dict(causal=True)),
    ("f16_d128", "f16", 1, 8, 4, 200, 333, 128, dict()),
    ("bf16_d128_wide_forward", "bf16", 4, 8, 2, 2048, 2048, 128, dict(causal=True)),      # fwd3 (64 rows per wave) on a chip-filling grid
    ("bf16_d64_split_keys", "bf16", 1, 4, 2, 40, 2500, 64, dict()),                         # split-key forward + combine
    ("f32_d32_mask", "f32", 2, 6, 3, 64, 100, 32, dict(mask=True)),
    ("f16_d64_bias", "f16", 1, 4, 2, 100, 150, 64, dict(bias=True)),
]


@pytest.mark.parametrize("name,dtype,B,H,Hk,N,M,D,kw", FWD_EQ, ids=[c[0] for c in FWD_EQ])
def test_gqa_forward_bit_identical_to_expanded_kv(name, dtype, B, H, Hk, N, M, D, kw):
    from flash_cosine_sim_attention_amd import _lib
    q, k, v, do, mask, bias = _inputs(dtype, B, H, Hk, N, M, D, kw, seed=11)
    G = H // Hk
    for form in ((1, 0) if D == 128 else (1,)):          # D = 128: both forward forms, pinned
        prev = _lib.forward_form(form)
        try:
            o, *_ = _run(q, k, v, do, mask, bias, kw, grads=False)
            oe, *_ = _run(q, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1), do, mask, bias, kw, grads=False)
        finally:
            _lib.forward_form(prev)
        assert torch.equal(o, oe), (name, form)


def test_gqa_expanded_gradients_match_group_sums():
    """dk / dv of the GQA call against the expanded-K/V call's gradients summed over each group (the same math, other kernels)"""
    dtype, B, H, Hk, N, M, D = "bf16", 2, 8, 2, 256, 256, 64
    q, k, v, do, mask, bias = _inputs(dtype, B, H, Hk, N, M, D, {}, seed=5)
    G = H // Hk
    _, dqe, dke, dve, _ = _run(q, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1), do, None, None, {})
    bar = T.GRAD_TOL[dtype] * T.SPLIT_GRAD_FACTOR[dtype]
    for form in (0, 2):
        with kv_form(form):
            _, dq, dk, dv, _ = _run(q, k, v, do, None, None, {})
        assert torch.equal(dq, dqe)
        for nm, g, e in (("dk", dk, dke), ("dv", dv, dve)):
            ref = _np(e).reshape(B, Hk, G, M, D).sum(2)
            assert T.check(f"gqa/expanded-sum/{nm}", dtype, _rel(_np(g), ref), bar), (form, nm)


@pytest.mark.parametrize("form", [0, 2])
@pytest.mark.parametrize("causal", [False, True])
def test_gqa_backward_deterministic(form, causal):
    q, k, v, do, _, _ = _inputs("bf16", 2, 8, 2, 333, 333, 128, {}, seed=3)
    kw = dict(causal=causal)
    with kv_form(form):
        a = _run(q, k, v, do, None, None, kw)
        b = _run(q, k, v, do, None, None, kw)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)


def _kernels_of_backward(q, k, v, do, kw):
    from flash_cosine_sim_attention_amd import _lib
    import flash_cosine_sim_attention_amd as F
    qq, kk, vv = (t.detach().clone().requires_grad_() for t in (q, k, v))
    o = F.flash_cosine_sim_attention(qq, kk, vv, **kw)
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    try:
        o.backward(do)
        torch.cuda.synchronize()
        names = {s["name"] for s in _lib.profile_collect()}
    finally:
        _lib.profile_enable(False)
    return names, (qq.grad, kk.grad, vv.grad)


def test_gqa_automatic_form_on_a_chip_filling_grid_is_the_sweep():
    """(4, 16, Hk 8, 2048, 64) bf16: the sweep grid (batch x K/V heads x 256-key tiles = 256 workgroups) covers the chip, so the automatic
    form is the group sweep -- no finalize launch, results bit-identical to the pinned sweep -- and it agrees with the slab route"""
    dtype, B, H, Hk, N, D = "bf16", 4, 16, 8, 2048, 64
    q, k, v, do, _, _ = _inputs(dtype, B, H, Hk, N, N, D, {}, seed=9)
    with kv_form(1):
        names, auto = _kernels_of_backward(q, k, v, do, {})
    assert "bwd_dkv" in names and "finalize" not in names, names
    with kv_form(2):
        _, sweep = _kernels_of_backward(q, k, v, do, {})
    with kv_form(0):
        names0, slab = _kernels_of_backward(q, k, v, do, {})
    assert "finalize" in names0, names0
    for a, s in zip(auto, sweep):
        assert torch.equal(a, s)
    bar = T.GRAD_TOL[dtype] * T.SPLIT_GRAD_FACTOR[dtype]
    for nm, a, s in zip(("dq", "dk", "dv"), auto, slab):
        assert T.check(f"gqa/auto-vs-slab/{nm}", dtype, _rel(_np(a), _np(s)), bar), nm
    # one (batch, K/V head) slice against the oracle
    G = H // Hk
    sl = lambda t: t[3:4]
    nq, ndo = _np(sl(q))[:, 2 * G:3 * G], _np(sl(do))[:, 2 * G:3 * G]
    nk, nv = np.repeat(_np(sl(k))[:, 2:3], G, axis=1), np.repeat(_np(sl(v))[:, 2:3], G, axis=1)
    rdq, rdk, rdv, _ = O.attention_backward(ndo, nq, nk, nv)
    assert T.check("gqa/auto/dk-slice", dtype, _rel(_np(auto[1])[3:4, 2:3], rdk.sum(1, keepdims=True)), bar)
    assert T.check("gqa/auto/dv-slice", dtype, _rel(_np(auto[2])[3:4, 2:3], rdv.sum(1, keepdims=True)), bar)


def test_gqa_sweep_takes_no_finalize_and_slab_route_does():
    q, k, v, do, _, _ = _inputs("f16", 1, 8, 2, 300, 300, 64, {}, seed=4)
    with kv_form(2):
        names, _ = _kernels_of_backward(q, k, v, do, dict(causal=True))
    assert "finalize" not in names, names
    with kv_form(0):
        names, _ = _kernels_of_backward(q, k, v, do, dict(causal=True))
    assert "finalize" in names, names


# ---- buffer bounds through the C ABI (see tests/test_gpu_buffer_bounds.py for the method) ------------------------------------------
FILL, GUARD = 0xFF, 4096


class _Arena:
    def __init__(self, nbytes):
        self.buf = torch.full((nbytes,), FILL, device="cuda", dtype=torch.uint8)
        self.off, self.used = GUARD, []

    def take(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        off = (self.off + 255) // 256 * 256
        assert off + n + GUARD <= self.buf.numel(), "arena too small"
        self.used.append((off, n))
        self.off = off + n + GUARD
        return self.buf[off:off + n].view(dtype).view(shape)

    def guards_intact(self):
        keep = torch.ones(self.buf.numel(), device="cuda", dtype=torch.bool)
        for off, n in self.used:
            keep[off:off + n] = False
        return bool((self.buf[keep] == FILL).all().item())


BOUNDS = [
    ("bf16_d64_causal_sweep", "bf16", 2, 8, 2, 333, 333, 64, dict(causal=True), 2),
    ("bf16_d64_causal_slabs", "bf16", 2, 8, 2, 333, 333, 64, dict(causal=True), 0),
    ("f16_d128_mask_sweep", "f16", 1, 6, 2, 130, 515, 128, dict(mask=True), 2),
    ("f16_d128_mask_slabs", "f16", 1, 6, 2, 130, 515, 128, dict(mask=True), 0),
    ("bf16_d64_split_queries_slabs", "bf16", 1, 4, 2, 3000, 200, 64, dict(), 1),
    ("bf16_d64_bias_slabs", "bf16", 1, 4, 2, 200, 260, 64, dict(bias=True), 2),
    ("f32_d32_causal", "f32", 1, 4, 2, 100, 190, 32, dict(causal=True), 1),
    ("bf16_d96_groups2", "bf16", 1, 4, 2, 200, 129, 96, dict(groups=2, scale=4.0), 2),
]


@pytest.mark.parametrize("name,dtype,B,H,Hk,N,M,D,kw,form", BOUNDS, ids=[c[0] for c in BOUNDS])
def test_gqa_calls_stay_inside_their_buffers(name, dtype, B, H, Hk, N, M, D, kw, form):
    from flash_cosine_sim_attention_amd import _lib
    lib = _lib.load()
    dt = DT[dtype]
    causal, groups, scale = kw.get("causal", False), kw.get("groups", 1), kw.get("scale", 8.0)
    with kv_form(form):
        prob = _lib.problem(dt, (B, H, Hk, N, M, D), causal, False, True, groups, scale)
        fws_n = int(lib.fcsa_forward_workspace_bytes(C.byref(prob)))
        bws_n = int(lib.fcsa_backward_workspace_bytes(C.byref(prob)))
        es = torch.empty((), dtype=dt).element_size()
        nbias = H * N * M if kw.get("bias") else 0
        ar = _Arena((6 * B * H * N * D + 7 * B * Hk * M * D + 2 * nbias) * es + (B * H * N * (1 + groups) + B * Hk * M * groups) * 4
                    + B * M + fws_n + bws_n + 40 * (GUARD + 256))
        g = torch.Generator(device="cuda").manual_seed(abs(hash(name)) % 10000)

        def rnd(shape):
            t = ar.take(shape, dt)
            t.copy_(torch.randn(shape, device="cuda", dtype=torch.float32, generator=g).to(dt))
            return t

        q, k, v, do = rnd((B, H, N, D)), rnd((B, Hk, M, D)), rnd((B, Hk, M, D)), rnd((B, H, N, D))
        mk = None
        if kw.get("mask"):
            mk = ar.take((B, M), torch.bool)
            mk.copy_(torch.rand((B, M), device="cuda", generator=g) > 0.3)
            mk[:, 0] = True
        ab = None
        if nbias:
            ab = ar.take((H, N, M), dt)
            ab.copy_((0.5 * torch.randn(ab.shape, device="cuda", generator=g)).to(dt))
        inputs = [t for t in (q, k, v, do, mk, ab) if t is not None]
        before = [t.clone() for t in inputs]
        o, inv_l = ar.take((B, H, N, D), dt), ar.take((B, H, N), torch.float32)
        qn, kn = ar.take((B, H, N, D), dt), ar.take((B, Hk, M, D), dt)
        rq, rk = ar.take((B, H, N, groups), torch.float32), ar.take((B, Hk, M, groups), torch.float32)
        fws = ar.take((fws_n,), torch.uint8) if fws_n else None
        ptr = lambda t: None if t is None else t.data_ptr()
        stream = torch.cuda.current_stream().cuda_stream
        norm = _lib.NormState(ptr(qn), ptr(kn), ptr(rq), ptr(rk))
        fa = _lib.ForwardArgs(prob, _lib.tensor4(q), _lib.tensor4(k), _lib.tensor4(v), _lib.tensor4(o), ptr(inv_l), ptr(mk), ptr(ab),
                              norm, ptr(fws), fws_n, stream)
        _lib.check(lib.fcsa_forward(C.byref(fa)), "fcsa_forward")
        ws = ar.take((max(bws_n, 1),), torch.uint8)
        dq, dk, dv = ar.take((B, H, N, D), dt), ar.take((B, Hk, M, D), dt), ar.take((B, Hk, M, D), dt)
        db = ar.take(ab.shape, dt) if ab is not None else None
        ba = _lib.BackwardArgs(prob, _lib.tensor4(do), _lib.tensor4(o), ptr(inv_l), _lib.tensor4(q), _lib.tensor4(k), _lib.tensor4(v),
                               ptr(mk), ptr(ab), norm, _lib.tensor4(dq), _lib.tensor4(dk), _lib.tensor4(dv), ptr(db), ws.data_ptr(), bws_n,
                               stream)
        _lib.check(lib.fcsa_backward(C.byref(ba)), "fcsa_backward")
        torch.cuda.synchronize()
    assert ar.guards_intact(), "a byte outside the call's buffers was written"
    for t, b in zip(inputs, before):
        assert torch.equal(t, b), "an input buffer was modified"
    outs = dict(o=o, dq=dq, dk=dk, dv=dv)
    if db is not None:
        outs["d_bias"] = db
    for nm, t in outs.items():
        bad = int((~torch.isfinite(t.float())).sum().item())
        assert bad == 0, f"{nm}: {bad} element(s) never written"


def test_gqa_opcheck():
    import flash_cosine_sim_attention_amd as F  # noqa: F401
    from flash_cosine_sim_attention_amd import _torch_ops
    fc = _torch_ops.load()
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn(2, 8, 64, 64, device="cuda", dtype=torch.bfloat16, generator=g)
    k = torch.randn(2, 2, 96, 64, device="cuda", dtype=torch.bfloat16, generator=g)
    v = torch.randn(2, 2, 96, 64, device="cuda", dtype=torch.bfloat16, generator=g)
    torch.library.opcheck(fc.forward, (q, k, v, None, None, False, 8.0, True, True, 1, True))
    o, inv_l, qn, kn, rq, rk = fc.forward(q, k, v, None, None, False, 8.0, True, True, 1, True)
    assert kn.shape == (2, 2, 96, 64) and rk.shape == (2, 2, 96, 1)
    do = torch.randn_like(q)
    torch.library.opcheck(fc.backward, (do, o, inv_l, q, k, v, None, None, qn, kn, rq, rk, False, 8.0, True, True, 1, False))
    dq, dk, dv, _ = fc.backward(do, o, inv_l, q, k, v, None, None, qn, kn, rq, rk, False, 8.0, True, True, 1, False)
    assert dk.shape == k.shape and dv.shape == v.shape
    torch.library.opcheck(fc.attention, (q.requires_grad_(), k.requires_grad_(), v.requires_grad_(), None, None, False, 8.0, True, True, 1))


def test_gqa_training_step_with_grad_scaler():
    import flash_cosine_sim_attention_amd as F
    torch.manual_seed(0)
    B, H, Hk, N, D = 2, 8, 2, 128, 64
    proj_q = torch.nn.Linear(D, H * D, device="cuda")
    proj_kv = torch.nn.Linear(D, 2 * Hk * D, device="cuda")
    opt = torch.optim.SGD(list(proj_q.parameters()) + list(proj_kv.parameters()), lr=1e-2)
    scaler = torch.amp.GradScaler("cuda")
    x = torch.randn(B, N, D, device="cuda")
    before = proj_kv.weight.detach().clone()
    with torch.autocast("cuda", dtype=torch.float16):
        q = proj_q(x).view(B, N, H, D).transpose(1, 2)
        k, v = proj_kv(x).view(B, N, 2, Hk, D).permute(2, 0, 3, 1, 4)
        o = F.flash_cosine_sim_attention(q.to(torch.float16), k.to(torch.float16), v.to(torch.float16), causal=True)
        loss = o.float().pow(2).mean()
    scaler.scale(loss).backward()
    assert proj_kv.weight.grad is not None and torch.isfinite(proj_kv.weight.grad).all()
    scaler.step(opt)
    scaler.update()
    assert not torch.equal(before, proj_kv.weight.detach())


def test_gqa_zero_keys():
    import flash_cosine_sim_attention_amd as F
    q = torch.randn(2, 8, 16, 64, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(2, 2, 0, 64, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(2, 2, 0, 64, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    o = F.flash_cosine_sim_attention(q, k, v)
    assert o.shape == q.shape and bool((o == 0).all())
    o.backward(torch.ones_like(o))
    assert q.grad.shape == q.shape and bool((q.grad == 0).all())
    assert k.grad.shape == k.shape and v.grad.shape == v.shape


@pytest.mark.parametrize("H,Hk", [(8, 3), (2, 3)])
def test_gqa_non_divisor_kv_heads_is_a_value_error(H, Hk):
    import flash_cosine_sim_attention_amd as F
    q = torch.randn(1, H, 16, 64, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(1, Hk, 16, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="k/v heads must divide q heads"):
        F.flash_cosine_sim_attention(q, k, k)
