"""Decoding against an fp8 (e4m3fn) key/value cache on the GPU (flash_cosine_sim_attention_with_kvcache with float8_e4m3fn caches,
fcsa_forward_kvcache_quant).

The cache means scale * code, and the result is what the 16-bit call computes on those values.  The reference is always the float64
oracle on code.double() * scale.double() (the caches as the call left them, so the append is part of it), under the policy of
test_gpu_kvcache.py::_verify and with its bars (tolerances.FWD_TOL, cases.logit_cond): every code is exact in f16 and bf16, so the inputs
of the arithmetic are exact and the fp8 kernel owes the accuracy of the 16-bit one -- no tolerance of its own.  The quantising append is
checked byte for byte against the rule  (x.float() / s).clamp(-448, 448).to(float8_e4m3fn)  computed on the CPU from copies."""
import numpy as np
import pytest
import torch

import cases as C
import test_gpu_kvcache as TK
from oracle import cosine_sim_oracle as O

pytestmark = pytest.mark.gpu

E4M3 = torch.float8_e4m3fn
DT = TK.DT


def _api():
    return TK._api()


def _rule(x, s):
    """the append rule on the CPU; x [..], s broadcastable (CPU float32)"""
    return (x.cpu().float() / s).clamp(-448, 448).to(E4M3).view(torch.uint8)


def _quantise(x, per=(2, 3)):
    """codes and per-(batch, head) amax / 448 scales of a float tensor [B, Hk, L, D] (CPU arithmetic, results on x's device)"""
    xc = x.cpu().float()
    s = (xc.abs().amax(dim=per) / 448).clamp_min(1e-6)
    codes = (xc / s[:, :, None, None]).clamp(-448, 448).to(E4M3)
    return codes.to(x.device), s.to(x.device)


def _seqs(kc, vc, ks, vs, lens, table=None):
    """positions [0, L_b) of every sequence as float64 [Hk, L_b, D]: code * scale[b]"""
    B = len(lens)
    ks, vs = (torch.as_tensor(s, dtype=torch.float32, device=kc.device).expand(B, kc.shape[1]).double() for s in (ks, vs))
    kq, vq = TK._seqs(kc.view(torch.uint8), vc.view(torch.uint8), lens, table)
    return ([k.view(E4M3).float().double() * ks[b][:, None, None] for b, k in enumerate(kq)],
            [v.view(E4M3).float().double() * vs[b][:, None, None] for b, v in enumerate(vq)])


def _inputs(dtype, B, H, Hk, N, cap, D, n_new, seed):
    """TK._inputs with the caches quantised under per-head amax scales"""
    q, kc, vc, kn, vn = TK._inputs(dtype, B, H, Hk, N, cap, D, n_new, seed)
    (k8, ks), (v8, vs) = _quantise(kc), _quantise(vc)
    return q, k8, v8, ks, vs, kn, vn


# ---- the grid -----------------------------------------------------------------------------------------------------------------------------

GRID = []
for i, (dtype, D, N) in enumerate([(dt, d, n) for dt in ("bf16", "f16") for d in (16, 32, 64, 96, 128) for n in (1, 3, 16)]):
    GRID.append((f"{dtype}_d{D}_n{N}", dtype, D, N, i % 2 == 0, (8, 2, 1)[i % 3]))


@pytest.mark.parametrize("name,dtype,D,N,causal,Hk", GRID, ids=[c[0] for c in GRID])
def test_fp8_grid(name, dtype, D, N, causal, Hk):
    H, B, cap = 8, 3, 300
    n_new = (0, 1, N)[(D // 16 + N) % 3]
    q, k8, v8, ks, vs, kn, vn = _inputs(dtype, B, H, Hk, N, cap, D, n_new, seed=sum(map(ord, name)))
    seq = [0, 17, cap - n_new] if N == 1 else [5, 130, cap - n_new]      # empty (N = 1, no append), one partial block, a full cache
    lens = [s + n_new for s in seq]
    with torch.no_grad():
        o = _api()(q, k8, v8, kn, vn, torch.tensor(seq, dtype=torch.int32, device="cuda"), causal=causal, k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    assert o.dtype == DT[dtype]
    kseq, vseq = _seqs(k8, v8, ks, vs, lens)
    TK._verify(dtype, o, q, kseq, vseq, dict(causal=causal), "fp8/" + name)
    for b, L in enumerate(lens):
        if L == 0:
            assert (o[b] == 0).all(), (name, b)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_fp8_every_code(dtype):
    """K and V caches that hold each of the 254 finite codes (subnormals and +-0 included), K under l2norm_qk, v_scale = 4 / 448 so that
    |v| <= 4, the range the bars were measured on.  Another encoding (fnuz: half the value) or a swapped byte order misses by factors."""
    B, H, Hk, N, D, cap = 2, 4, 2, 2, 64, 512
    g = torch.Generator().manual_seed(12)
    def codes():
        c = torch.randint(0, 256, (B, Hk, cap, D), dtype=torch.uint8, generator=g)
        c[:, :, :4] = torch.arange(256, dtype=torch.uint8).view(4, D)      # every byte value, in byte order, in every head
        c[(c & 0x7f) == 0x7f] = 0x01                                        # the two NaN codes -> the smallest subnormal
        return c
    ck, cv = codes(), codes()
    for c in (ck, cv):
        assert len(set(c.flatten().tolist())) == 254
    k8, v8 = ck.cuda().view(E4M3), cv.cuda().view(E4M3)
    q = torch.randn(B, H, N, D, generator=g).to(DT[dtype]).cuda()
    ks, vs = 0.25, 4.0 / 448
    for kw in (dict(causal=True), dict(causal=False, scale=4.0)):
        with torch.no_grad():
            o = _api()(q, k8, v8, cache_seqlens=torch.tensor([cap, 300], dtype=torch.int32, device="cuda"), k_scale=ks, v_scale=vs, **kw)
        torch.cuda.synchronize()
        kseq, vseq = _seqs(k8, v8, ks, vs, [cap, 300])
        assert max(float(v.abs().max()) for v in vseq) <= 4.0 * (1 + 1e-6)
        TK._verify(dtype, o, q, kseq, vseq, kw, f"fp8/every_code_{dtype}_{sorted(kw.items())}")


# ---- regimes ------------------------------------------------------------------------------------------------------------------------------

# Without a widened bar (cases.logit_cond == 1: scale * groups <= 16) the cases stay at scale * groups <= 8, the logit range of the default
# call (scale 8, one group) that the raw bars were calibrated on: the error the 16-bit rounding of q^, k^ leaves in a logit grows as
# scale * groups / sqrt(D), so scale * groups = 16 is the very edge of the unwidened bar.  Measured there (bf16, D = 64, groups 16,
# scale 1, N = 1, eight seeds): raw rel-L2 3.0e-3 ... 4.9e-3 on fp8 caches and 2.9e-3 ... 5.8e-3 for the 16-bit call on randn caches,
# against the 4.5e-3 bar -- and the fp8 call equals the 16-bit call on the same values bit for bit (test_fp8_equals_16bit_call_...), so
# that spread belongs to the case, not to either kernel.  Beyond 16 the per-row cases run with the bar that logit_cond widens.
REGIMES = [
    ("f16_scale8_groups2_per_row", "f16", 64, 4, 8, 2, dict(scale=8.0, groups=2, causal=True)),
    ("bf16_scale120_per_row", "bf16", 128, 1, 8, 8, dict(scale=120.0)),
    ("f16_static_scale4", "f16", 128, 2, 8, 2, dict(scale=4.0)),
    ("bf16_static_scale8_d96", "bf16", 96, 3, 8, 1, dict(scale=8.0, causal=True)),
    ("bf16_groups4", "bf16", 64, 3, 8, 2, dict(groups=4, scale=2.0, causal=True)),
    ("bf16_groups16_in_lane", "bf16", 64, 1, 4, 4, dict(groups=16, scale=0.5)),
    ("f16_groups16_in_lane_per_row", "f16", 64, 2, 4, 4, dict(groups=16, scale=1.0, causal=True)),
    ("f16_groups8_in_lane_d32", "f16", 32, 1, 4, 2, dict(groups=8, scale=1.0)),
    ("f16_groups2_d16", "f16", 16, 2, 4, 2, dict(groups=2, scale=2.0)),
    ("f16_no_l2norm", "f16", 64, 2, 4, 2, dict(l2norm_qk=False, scale=1.0, causal=True)),
    ("bf16_no_l2norm_d128", "bf16", 128, 1, 8, 2, dict(l2norm_qk=False, scale=2.0)),
    ("bf16_d96_groups3", "bf16", 96, 2, 4, 2, dict(groups=3, scale=2.0)),
    # D = 96 group widths that straddle a lane's fragment (48, 24, 12, 6, 3 features): the kernel's LDS form
    ("f16_d96_groups2_per_row", "f16", 96, 4, 8, 2, dict(groups=2, scale=8.0, causal=True)),
    ("bf16_d96_groups2", "bf16", 96, 1, 8, 8, dict(groups=2, scale=8.0)),
    ("bf16_d96_groups4", "bf16", 96, 3, 8, 2, dict(groups=4, scale=2.0, causal=True)),
    ("f16_d96_groups8", "f16", 96, 1, 4, 4, dict(groups=8, scale=1.0)),
    ("bf16_d96_groups16", "bf16", 96, 2, 4, 1, dict(groups=16, scale=0.5)),
    ("bf16_d96_groups32_per_row", "bf16", 96, 2, 8, 2, dict(groups=32, scale=4.0)),
    ("f16_d96_groups32", "f16", 96, 1, 4, 1, dict(groups=32, scale=0.25)),
]


@pytest.mark.parametrize("name,dtype,D,N,H,Hk,kw", REGIMES, ids=[c[0] for c in REGIMES])
def test_fp8_regimes(name, dtype, D, N, H, Hk, kw):
    B, cap = 2, 700
    l2 = kw.get("l2norm_qk", True)
    q, kc, vc, kn, vn = TK._inputs(dtype, B, H, Hk, N, cap, D, N, seed=sum(map(ord, name)))
    q, kc = TK._unit_normalised(q, kc, kw.get("groups", 1), l2)      # (l2norm_qk=False: unit-norm keys, so k_scale is about 1 / 448 / sqrt(D))
    _, kn = TK._unit_normalised(q, kn, 1, l2)
    (k8, ks), (v8, vs) = _quantise(kc), _quantise(vc)
    assert float((ks - 1).abs().min()) > 0                             # k_scale != 1 everywhere
    seq = [600, 33]
    with torch.no_grad():
        o = _api()(q, k8, v8, kn, vn, torch.tensor(seq, dtype=torch.int32, device="cuda"), k_scale=ks, v_scale=vs, **kw)
    torch.cuda.synchronize()
    kseq, vseq = _seqs(k8, v8, ks, vs, [s + N for s in seq])
    TK._verify(dtype, o, q, kseq, vseq, kw, "fp8/" + name)


@pytest.mark.parametrize("dtype,D,groups", [("bf16", 128, 1), ("f16", 64, 4), ("bf16", 96, 4)])
def test_fp8_k_scale_cancels_under_l2norm(dtype, D, groups):
    """the same codes under k_scale 1.0 and 0.37: one reference (the scale cancels in exact arithmetic), both within the bars"""
    B, H, Hk, N, cap = 2, 8, 2, 2, 400
    q, k8, v8, ks, vs, _, _ = _inputs(dtype, B, H, Hk, N, cap, D, 0, seed=21)
    sl = torch.tensor([cap, 123], dtype=torch.int32, device="cuda")
    kw = dict(causal=True, groups=groups, scale=8.0 / groups)      # scale * groups = 8: see the note above REGIMES
    kseq, vseq = _seqs(k8, v8, 1.0, vs, [cap, 123])
    for s in (1.0, 0.37, torch.tensor([[1.0, 0.37], [3.0, 0.01]])):
        with torch.no_grad():
            o = _api()(q, k8, v8, cache_seqlens=sl, k_scale=s, v_scale=vs, **kw)
        torch.cuda.synchronize()
        TK._verify(dtype, o, q, kseq, vseq, kw, f"fp8/k_scale_{dtype}_d{D}_{s if isinstance(s, float) else 'b_hk'}")


def _pow2_quantise(x):
    """codes, power-of-two per-head scales and the 16-bit tensor that holds scale * code exactly"""
    xc = x.cpu().float()
    s = torch.exp2(torch.ceil(torch.log2(xc.abs().amax(dim=(2, 3)) / 448)))
    codes = (xc / s[:, :, None, None]).clamp(-448, 448).to(E4M3)
    return codes.to(x.device), s.to(x.device), (codes.float() * s[:, :, None, None]).to(x.dtype).to(x.device)


SAME = [("bf16_d128", "bf16", 128, 1, 8, 2, dict(causal=True)),
        ("f16_d64_per_row", "f16", 64, 3, 8, 2, dict(scale=8.0, groups=2, causal=True)),
        ("bf16_d64_groups16_scale1", "bf16", 64, 1, 4, 4, dict(groups=16, scale=1.0)),
        ("bf16_d96_groups4_lds_form", "bf16", 96, 3, 8, 2, dict(groups=4, scale=2.0, causal=True)),
        ("f16_d16", "f16", 16, 16, 2, 1, dict()),
        ("bf16_d32_no_l2norm", "bf16", 32, 2, 4, 2, dict(l2norm_qk=False, scale=1.0, causal=True)),
        ("f16_d128_window", "f16", 128, 2, 8, 2, dict(causal=True, window_size=(100, 0)))]


@pytest.mark.parametrize("name,dtype,D,N,H,Hk,kw", SAME, ids=[c[0] for c in SAME])
def test_fp8_equals_16bit_call_on_the_same_values_bit_for_bit(name, dtype, D, N, H, Hk, kw):
    """Under power-of-two scales a 16-bit cache holds scale * code exactly and every scaling by k_scale / v_scale is exact in float32, so
    the fp8 call must return the bits of the 16-bit call on that cache -- the appended rows (exactly representable: code * scale)
    included.  This is the sense in which the fp8 kernel owes the accuracy of the 16-bit one."""
    B, cap = 2, 700
    l2 = kw.get("l2norm_qk", True)
    q, kc, vc, kn, vn = TK._inputs(dtype, B, H, Hk, N, cap, D, N, seed=sum(map(ord, name)))
    q, kc = TK._unit_normalised(q, kc, kw.get("groups", 1), l2)
    (k8, ks, k16), (v8, vs, v16) = _pow2_quantise(kc), _pow2_quantise(vc)
    kn16 = (_rule(kn, ks.cpu()[:, :, None, None]).view(E4M3).float() * ks.cpu()[:, :, None, None]).to(DT[dtype]).cuda()
    vn16 = (_rule(vn, vs.cpu()[:, :, None, None]).view(E4M3).float() * vs.cpu()[:, :, None, None]).to(DT[dtype]).cuda()
    sl = torch.tensor([600, 33], dtype=torch.int32, device="cuda")
    with torch.no_grad():
        o8 = _api()(q, k8, v8, kn16, vn16, sl, k_scale=ks, v_scale=vs, **kw)
        o16 = _api()(q, k16, v16, kn16, vn16, sl, **kw)
    torch.cuda.synchronize()
    assert torch.equal(o8, o16), (name, float((o8.float() - o16.float()).abs().max()))
    assert torch.equal((k8.float() * ks[:, :, None, None]).to(DT[dtype]), k16) and torch.equal((v8.float() * vs[:, :, None, None]).to(DT[dtype]), v16)


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f16", 16), ("bf16", 128)])
def test_fp8_paged_equals_contiguous(dtype, D):
    B, H, Hk, N, page, mb = 3, 8, 2, 2, 32, 6
    cap = page * mb
    q, k8, v8, ks, vs, kn, vn = _inputs(dtype, B, H, Hk, N, cap, D, N, seed=7)
    seq = [0, 70, cap - N]
    nb = B * mb + 5
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(3))[:B * mb].reshape(B, mb).to(torch.int32)
    # the vLLM layout [num_blocks, page, Hk, D] passed transposed; pages outside every table hold NaN codes
    pool_k = torch.full((nb, page, Hk, D), 0x7f, device="cuda", dtype=torch.uint8)
    pool_v = torch.full_like(pool_k, 0xff)
    ku, vu = k8.view(torch.uint8), v8.view(torch.uint8)
    for b in range(B):
        for i in range(mb):
            pool_k[int(perm[b, i])] = ku[b, :, i * page:(i + 1) * page].transpose(0, 1)
            pool_v[int(perm[b, i])] = vu[b, :, i * page:(i + 1) * page].transpose(0, 1)
    kpool, vpool = pool_k.view(E4M3).transpose(1, 2), pool_v.view(E4M3).transpose(1, 2)
    sl = torch.tensor(seq, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        oc = _api()(q, k8, v8, kn, vn, sl, causal=True, k_scale=ks, v_scale=vs)
        op = _api()(q, kpool, vpool, kn, vn, sl, block_table=perm.cuda(), causal=True, k_scale=ks, v_scale=vs)
        oh = _api()(q, kpool, vpool, kn, vn, torch.tensor(seq, dtype=torch.int32), block_table=perm, causal=True, k_scale=ks.cpu(), v_scale=vs.cpu())
    torch.cuda.synchronize()
    assert torch.equal(oc, op) and torch.equal(op, oh)
    kseq, vseq = _seqs(kpool, vpool, ks, vs, [s + N for s in seq], perm)
    TK._verify(dtype, op, q, kseq, vseq, dict(causal=True), f"fp8/paged_{dtype}_d{D}")
    unused = sorted(set(range(nb)) - set(perm.flatten().tolist()))
    assert (pool_k[unused] == 0x7f).all() and (pool_v[unused] == 0xff).all()
    for b in range(B):                                  # the paged append wrote what the contiguous one wrote
        for t in range(N):
            pos = seq[b] + t
            blk = int(perm[b, pos // page])
            assert torch.equal(pool_k[blk, pos % page], ku[b, :, pos]) and torch.equal(pool_v[blk, pos % page], vu[b, :, pos])


def _special(dtype, s, n):
    """n values of `dtype` whose quotients by s cover: beyond +-448, exact ties between neighbouring codes (normal and subnormal), the
    subnormal range, magnitudes that round to zero, +-0"""
    codes = torch.arange(256, dtype=torch.uint8).view(E4M3).float()
    pos = torch.sort(codes[torch.isfinite(codes) & (codes >= 0)]).values
    ties = (pos[:-1] + pos[1:]) / 2
    vals = torch.cat([torch.tensor([0.0, -0.0, 449.0, 464.0, 480.0, 1e4, -449.0, -464.0, -1e4, 2.0 ** -10, 2.0 ** -11, 3 * 2.0 ** -11, -(2.0 ** -10),
                                    1e-8, -1e-8]), ties, -ties, pos, -pos])
    g = torch.Generator().manual_seed(int(s * 1000) + n)
    fill = torch.randn(max(n - vals.numel(), 0), generator=g) * 200
    return (torch.cat([vals, fill])[:n] * s).to(dtype)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("D", [16, 96])
def test_fp8_append_bytes_and_guard_regions(dtype, D):
    """A guard-filled arena around [B, capacity, Hk, D]-transposed caches: the appended slots hold the rule's bytes (computed on the CPU
    from copies), every other byte -- valid slot, unused slot (NaN codes) or guard band -- keeps its value, and the appended rows are seen
    by the same call's attention."""
    B, H, Hk, N, cap, guard = 3, 4, 2, 40, 100, 4096      # N: appended rows (two queries attend)
    dt = DT[dtype]
    q = torch.randn(B, H, 2, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8)).to(dt)
    ks = torch.tensor([[1.0, 0.37], [2.0 ** -4, 3.0], [0.011, 1.0]])
    vs = torch.tensor([4.0 / 448, 2.0 / 448])             # |v| <= 4 over the whole code range: the range the bars were measured on
    kn = torch.stack([torch.stack([_special(dt, float(ks[b, h]), N * D).view(N, D) for h in range(Hk)]) for b in range(B)]).cuda()
    vn = torch.stack([torch.stack([_special(dt, float(vs[h]), N * D).flip(0).view(N, D) for h in range(Hk)]) for b in range(B)]).cuda()
    n = B * cap * Hk * D
    arena_k = torch.full((2 * guard + n,), 0xa5, device="cuda", dtype=torch.uint8)
    arena_v = torch.full_like(arena_k, 0x5a)
    ku = arena_k[guard:guard + n].view(B, cap, Hk, D).transpose(1, 2)
    vu = arena_v[guard:guard + n].view(B, cap, Hk, D).transpose(1, 2)
    seq = [0, 40, cap - N]
    g = torch.Generator().manual_seed(4)
    ku.copy_(torch.randint(0, 0x7f, (B, Hk, cap, D), dtype=torch.uint8, generator=g))
    vu.copy_(torch.randint(0, 0x7f, (B, Hk, cap, D), dtype=torch.uint8, generator=g))
    for b, s in enumerate(seq):                          # slots beyond each sequence's length hold NaN codes: they must never reach the output
        ku[b, :, s:] = 0x7f
        vu[b, :, s:] = 0xff
    before_k, before_v = ku.clone(), vu.clone()
    with torch.no_grad():
        o = _api()(q, ku.view(E4M3), vu.view(E4M3), kn, vn, torch.tensor(seq, dtype=torch.int32, device="cuda"), k_scale=ks.cuda(), v_scale=vs.cuda())
    torch.cuda.synchronize()
    assert torch.isfinite(o).all()
    assert (arena_k[:guard] == 0xa5).all() and (arena_k[-guard:] == 0xa5).all()
    assert (arena_v[:guard] == 0x5a).all() and (arena_v[-guard:] == 0x5a).all()
    exp_k, exp_v = before_k.cpu(), before_v.cpu()
    for b, s in enumerate(seq):
        exp_k[b, :, s:s + N] = _rule(kn[b], ks[b][:, None, None])
        exp_v[b, :, s:s + N] = _rule(vn[b], vs[:, None, None])
    for nm, got, exp, src, sc in (("k", ku.cpu(), exp_k, kn, ks[:, :, None, None]), ("v", vu.cpu(), exp_v, vn, vs[None, :, None, None])):
        bad = (got != exp).nonzero()
        detail = [(tuple(i.tolist()), hex(int(got[tuple(i)])), hex(int(exp[tuple(i)]))) for i in bad[:8]]
        assert bad.numel() == 0, (nm, len(bad), detail)
    assert {0x7e, 0xfe, 0x00, 0x80, 0x01} <= set(exp_k[0, 0, :N].flatten().tolist())      # saturated, +-0 and subnormal codes were written
    kseq, vseq = _seqs(ku.view(E4M3), vu.view(E4M3), ks, vs, [s + N for s in seq])
    TK._verify(dtype, o, q, kseq, vseq, {}, f"fp8/guard_{dtype}_d{D}")
    # sequence 0 holds nothing but the appended rows, and its output is not zero: the call's attention saw them
    assert float(o[0].float().abs().max()) > 0


def test_fp8_append_nan_stays_nan_and_capacity_drops():
    B, H, Hk, N, D, cap = 1, 2, 1, 3, 32, 64
    q = torch.ones(B, H, 1, D, device="cuda").bfloat16()
    k8 = torch.zeros(B, Hk, cap, D, device="cuda", dtype=torch.uint8).view(E4M3)
    v8 = torch.zeros(B, Hk, cap, D, device="cuda", dtype=torch.uint8).view(E4M3)
    kn = torch.ones(B, Hk, N, D, device="cuda").bfloat16()
    kn[0, 0, 0, 5] = float("nan")
    vn = kn.clone()
    # a device table is trusted: 2 of the 3 rows lie beyond the capacity and are dropped
    _api()(q, k8, v8, kn, vn, torch.tensor([cap - 1], dtype=torch.int32, device="cuda"), k_scale=0.5, v_scale=0.5)
    torch.cuda.synchronize()
    ku = k8.view(torch.uint8).cpu()
    assert int(ku[0, 0, cap - 1, 5]) & 0x7f == 0x7f                      # NaN stays NaN
    assert (ku[0, 0, cap - 1, :5] == 0x40).all() and (ku[0, 0, cap - 1, 6:] == 0x40).all()      # 1 / 0.5 = 2.0
    assert (ku[0, 0, :cap - 1] == 0).all()


@pytest.mark.parametrize("layout", ["contiguous", "paged"])
@pytest.mark.parametrize("call", ["rectangular", "ragged"])
@pytest.mark.parametrize("cache", ["bf16", "fp8"])
def test_append_rule_on_every_form(cache, call, layout):
    """The append's one rule -- start at cache_seqlens, drop at the capacity, through the block table when paged -- over every append entry
    point.  Sequence 0 holds capacity - 1 positions and brings 3 rows: one lands in the last slot, two cross the capacity and are dropped.
    Sequence 1 holds 5 and takes all of its rows.  The caches live in sentinel-filled arenas (NaN; for fp8 the byte 0xff, a code no finite
    input quantises to) with a guard of one whole sequence's cache on either side, and sequence 0's last page is not the last in memory,
    so a row that was not dropped would land inside the arena.  Written slots equal the new rows bit for bit (fp8: the codes of the CPU
    rule), every other byte of the arenas keeps its bits, and o is finite."""
    import flash_cosine_sim_attention_amd as F
    B, H, Hk, D, cap, page, blocks = 2, 2, 1, 32, 32, 16, 4
    fp8, ragged, is_paged = cache == "fp8", call == "ragged", layout == "paged"
    seq, counts = [cap - 1, 5], ([3, 1] if ragged else [3, 3])
    g = torch.Generator().manual_seed(7)
    rnd = lambda *shape: torch.randn(*shape, generator=g).bfloat16()
    guard = Hk * cap * D
    ks, vs = torch.tensor([[0.75], [1.5]]), torch.tensor([[0.3], [2.0]])
    table = [[2, 0], [3, 1]] if is_paged else None           # shuffled; sequence 0's last page is block 0
    shape = (blocks, Hk, page, D) if is_paged else (B, Hk, cap, D)
    n = shape[0] * shape[1] * shape[2] * shape[3]

    def slot(c, b, pos):
        return c[table[b][pos // page], :, pos % page] if is_paged else c[b, :, pos]

    def code(x, s, b):       # what a slot holds of row x [Hk, D] of sequence b: the row itself, or its codes under the (b, kvh) scales
        return _rule(x, s[b][:, None]) if fp8 else x

    arenas, caches = [], []
    for s in (ks, vs):
        arena = torch.full((2 * guard + n,), 0xff, dtype=torch.uint8) if fp8 else torch.full((2 * guard + n,), float("nan"), dtype=torch.bfloat16)
        c = arena[guard:guard + n].view(shape)
        for b in range(B):
            for pos in range(seq[b]):
                slot(c, b, pos).copy_(code(rnd(Hk, D), s, b))
        arenas.append(arena)
        caches.append(c)
    total = sum(counts)
    q, kn, vn = rnd(total, H, D), rnd(total, Hk, D), rnd(total, Hk, D)
    expect = [a.clone() for a in arenas]
    for e, new, s in zip(expect, (kn, vn), (ks, vs)):
        c = e[guard:guard + n].view(shape)
        for b in range(B):
            for i in range(counts[b]):
                if seq[b] + i < cap:
                    slot(c, b, seq[b] + i).copy_(code(new[sum(counts[:b]) + i], s, b))
    dev = [a.cuda() for a in arenas]
    kc, vc = (a[guard:guard + n].view(shape) for a in dev)
    if fp8:
        kc, vc = kc.view(E4M3), vc.view(E4M3)
    kw = dict(cache_seqlens=torch.tensor(seq, dtype=torch.int32, device="cuda"),
              block_table=torch.tensor(table, dtype=torch.int32, device="cuda") if is_paged else None)
    if fp8:
        kw.update(k_scale=ks.cuda(), v_scale=vs.cuda())
    packed = lambda t: t.cuda()
    rect = lambda t: t.view(B, 3, -1, D).transpose(1, 2).contiguous().cuda()      # [B * 3, heads, D] -> [B, heads, 3, D]
    with torch.no_grad():
        if ragged:
            cu = torch.tensor([0, 3, 4], dtype=torch.int32, device="cuda")
            o = F.flash_cosine_sim_attention_varlen_with_kvcache(packed(q), kc, vc, cu, packed(kn), packed(vn), **kw)
        else:
            o = F.flash_cosine_sim_attention_with_kvcache(rect(q), kc, vc, rect(kn), rect(vn), **kw)
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.uint8) if fp8 else t.view(torch.int16)
    for name, got, want, before in zip("kv", dev, expect, arenas):
        got = bits(got.cpu())
        assert torch.equal(got[:guard], bits(before)[:guard]) and torch.equal(got[-guard:], bits(before)[-guard:]), f"{name}: a guard band was written"
        diff = (got != bits(want)).nonzero().flatten()
        assert diff.numel() == 0, f"{name}: {diff.numel()} elements differ from the expected arena, first at {int(diff[0]) - guard} of the cache"
        assert (bits(want) != bits(before)).any()      # the call did append
    assert torch.isfinite(o).all()


# ---- window -------------------------------------------------------------------------------------------------------------------------------

def _band(N, M, left, right, causal):
    i = np.arange(N)[:, None] + (M - N)
    j = np.arange(M)[None]
    ok = np.ones((N, M), bool)
    if left >= 0:
        ok &= j >= i - left
    r = 0 if causal else right
    if r >= 0:
        ok &= j <= i + r
    return np.where(ok, 0.0, -np.inf)[None]


@pytest.mark.parametrize("dtype,D,left,right,causal", [("bf16", 128, 100, 0, True), ("f16", 64, 37, 2, False), ("bf16", 32, 0, -1, False),
                                                        ("f16", 96, 300, 0, True)])
def test_fp8_window_against_oracle(dtype, D, left, right, causal):
    """static regime (scale 8, one group), both passes of _verify with the window as an additive bias of the oracle"""
    B, H, Hk, N, cap = 3, 8, 2, 3, 700
    q, k8, v8, ks, vs, kn, vn = _inputs(dtype, B, H, Hk, N, cap, D, N, seed=31 + D)
    seq = [0, 333, cap - N]
    lens = [s + N for s in seq]
    with torch.no_grad():
        o = _api()(q, k8, v8, kn, vn, torch.tensor(seq, dtype=torch.int32, device="cuda"), causal=causal, window_size=(left, right),
                   k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    kseq, vseq = _seqs(k8, v8, ks, vs, lens)
    G = H // Hk
    for operand_dtype, cond in ((None, C.logit_cond(dtype, 8.0, 1, True)), (dtype, 1.0)):
        ref = np.zeros(q.shape)
        for b, L in enumerate(lens):
            kr, vr = (np.repeat(TK._np(x)[None], G, axis=1) for x in (kseq[b], vseq[b]))
            ref[b] = O.attention_forward_stats(TK._np(q[b:b + 1]), kr, vr, scale=8.0, groups=1, causal=causal, l2norm_qk=True,
                                               attn_bias=np.repeat(_band(N, L, left, right, causal), H, axis=0), eps=1e-10,
                                               operand_dtype=operand_dtype)[0][0]
        TK._check(dtype, o, ref, f"fp8/window_{dtype}_d{D}_{left}_{right}/{'raw' if operand_dtype is None else 'operands'}", cond)


@pytest.mark.parametrize("dtype,D", [("bf16", 128), ("f16", 32)])
def test_fp8_window_that_hides_nothing_is_the_plain_call(dtype, D):
    B, H, Hk, N, cap = 2, 4, 2, 2, 300
    q, k8, v8, ks, vs, _, _ = _inputs(dtype, B, H, Hk, N, cap, D, 0, seed=41)
    sl = torch.tensor([cap, 77], dtype=torch.int32, device="cuda")
    with torch.no_grad():
        for causal in (True, False):
            plain = _api()(q, k8, v8, cache_seqlens=sl, causal=causal, k_scale=ks, v_scale=vs)
            for win in ((cap, -1), (-1, 0) if causal else (-1, N - 1), (cap - 1, N)):
                assert torch.equal(plain, _api()(q, k8, v8, cache_seqlens=sl, causal=causal, window_size=win, k_scale=ks, v_scale=vs)), (causal, win)
        # ... and one that does hide something differs
        assert not torch.equal(plain, _api()(q, k8, v8, cache_seqlens=sl, causal=False, window_size=(5, 0), k_scale=ks, v_scale=vs))


# ---- tables and tracing -------------------------------------------------------------------------------------------------------------------

def test_fp8_host_device_int_seqlens():
    B, H, Hk, N, D, cap = 4, 8, 8, 1, 128, 1000
    q, k8, v8, ks, vs, _, _ = _inputs("bf16", B, H, Hk, N, cap, D, 0, seed=5)
    seq = [0, 1, 999, 1000]
    f = lambda **kw: _api()(q, k8, v8, causal=True, k_scale=ks, v_scale=vs, **kw)
    with torch.no_grad():
        od = f(cache_seqlens=torch.tensor(seq, dtype=torch.int32, device="cuda"))
        oh = f(cache_seqlens=torch.tensor(seq, dtype=torch.int32), max_seqlen_k=1000)
        of = f()
        oi = f(cache_seqlens=1000)
        small = f(cache_seqlens=torch.tensor(seq, dtype=torch.int32, device="cuda"), max_seqlen_k=64)
    torch.cuda.synchronize()
    assert torch.equal(od, oh) and torch.equal(of, oi)
    assert (od[0] == 0).all() and torch.equal(od[3], of[3])
    kseq, vseq = _seqs(k8, v8, ks, vs, seq)
    TK._verify("bf16", od, q, kseq, vseq, dict(causal=True), "fp8/ragged")
    TK._verify("bf16", small, q, kseq, vseq, dict(causal=True), "fp8/ragged_small_grid")


def test_fp8_refusals_on_the_gpu():
    q, k8, v8, ks, vs, kn, vn = _inputs("bf16", 1, 2, 2, 1, 64, 32, 1, seed=1)
    with pytest.raises(TypeError, match="one fp8 cache and one"):
        _api()(q, k8, v8.to(torch.bfloat16), cache_seqlens=3)
    with pytest.raises(TypeError, match="not supported"):
        _api()(q, k8.float().to(torch.float8_e5m2), v8.float().to(torch.float8_e5m2), cache_seqlens=3)
    with pytest.raises(TypeError, match="scales belong to"):
        _api()(q, k8.to(torch.bfloat16), v8.to(torch.bfloat16), cache_seqlens=3, k_scale=ks)
    with pytest.raises(TypeError, match="float16 or bfloat16"):
        _api()(q.float(), k8, v8, cache_seqlens=3)
    with pytest.raises(RuntimeError):
        _api()(q.clone().requires_grad_(), k8, v8, cache_seqlens=3)


def test_fp8_opcheck():
    import flash_cosine_sim_attention_amd._torch_ops as ops
    fc = ops.load()
    q, k8, v8, ks, vs, kn, vn = _inputs("bf16", 2, 4, 2, 2, 64, 32, 2, seed=2)
    sl = torch.tensor([3, 40], dtype=torch.int32, device="cuda")
    one = torch.ones((), device="cuda")
    k8, v8 = k8.view(torch.uint8), v8.view(torch.uint8)          # the op takes the codes as bytes
    torch.library.opcheck(fc.kvcache_fp8_forward.default, (q, k8, v8, kn, vn, sl, None, ks, vs, 64, 8.0, True, True, 1, -1, -1))
    torch.library.opcheck(fc.kvcache_fp8_forward.default, (q, k8, v8, kn, vn, sl, None, one, vs[0].contiguous(), 64, 8.0, True, True, 1, 20, 0))
    tab = torch.tensor([[1, 0], [2, 3]], dtype=torch.int32, device="cuda")
    kp = torch.randint(0, 0x7f, (4, 2, 32, 32), dtype=torch.uint8, device="cuda")
    vp = torch.randint(0, 0x7f, (4, 2, 32, 32), dtype=torch.uint8, device="cuda")
    torch.library.opcheck(fc.kvcache_fp8_forward.default, (q, kp, vp, kn, vn, sl, tab, ks, vs, 64, 8.0, False, True, 1, -1, -1))


def test_fp8_graph_capture_and_replay():
    """device lengths, device scales and max_seqlen_k given: the call does not synchronise, so a step is captured and replayed with the
    lengths (and the inputs) changed between replays"""
    B, H, Hk, N, D, cap = 2, 8, 2, 1, 64, 512
    q, k8, v8, ks, vs, kn, vn = _inputs("bf16", B, H, Hk, N, cap, D, 1, seed=4)
    sl = torch.tensor([10, 300], dtype=torch.int32, device="cuda")
    f = lambda kc, vc: _api()(q, kc, vc, kn, vn, sl, max_seqlen_k=cap, k_scale=ks, v_scale=vs)
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            f(k8, v8)                                             # warm-up (allocator, lazy init)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        k_eager, v_eager = k8.clone(), v8.clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = f(k8, v8)
        for step in range(3):
            q.copy_(torch.randn_like(q))
            kn.copy_(torch.randn_like(kn))
            vn.copy_(torch.randn_like(vn))
            sl.copy_(torch.tensor([11 + step, 301 + 2 * step], dtype=torch.int32))
            g.replay()
            ref = f(k_eager, v_eager)
            torch.cuda.synchronize()
            assert torch.equal(out, ref), step
            assert torch.equal(k8.view(torch.uint8), k_eager.view(torch.uint8)) and torch.equal(v8.view(torch.uint8), v_eager.view(torch.uint8)), step


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_fp8_many_splits_long_cache(dtype):
    """L >= 64k at D = 32 on a small grid: the split cap (128 splits), windows that end inside a 32-key block, ragged lengths; the static
    regime and (scale 16, groups 2) the per-row regime of float16"""
    B, H, Hk, N, cap, D = 3, 4, 1, 3, 66000, 32
    q, k8, v8, ks, vs, kn, vn = _inputs(dtype, B, H, Hk, N, cap, D, 2, seed=D + len(dtype))
    seq = [cap - 2, 65537, 553]
    for kw in (dict(causal=True), dict(scale=16.0, groups=2)):
        k_, v_ = k8.clone(), v8.clone()
        with torch.no_grad():
            o = _api()(q, k_, v_, kn, vn, torch.tensor(seq, dtype=torch.int32, device="cuda"), k_scale=ks, v_scale=vs, **kw)
        torch.cuda.synchronize()
        kseq, vseq = _seqs(k_, v_, ks, vs, [s + 2 for s in seq])
        TK._verify(dtype, o, q, kseq, vseq, kw, f"fp8/splits_{dtype}_{sorted(kw)}")
