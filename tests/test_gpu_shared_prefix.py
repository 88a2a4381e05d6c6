"""The shared-prefix decode step on the GPU (flash_cosine_sim_attention_with_shared_prefix): a prefix cached once, every sequence's own
cache behind it.

The result must be what the plain cache call gives on caches that each hold a COPY of the prefix in front of the sequence's own positions
(materialised here), and what the float64 oracle gives on those keys; prefix_len = 0 is the suffix call bit for bit; the append lands in the
sequences' own caches only; a paged pool may hold prefix and sequences side by side; fp8 caches pass through; the step can be captured in a
graph.  Composed-route bars: tests/tolerances_lse.py.  Under causal every sequence holds at least its own queries (N_b <= L_b), which the
causal cases get from the append, as a decode step does; the empty own cache (L_b = 0) is met by the non-causal cases."""
import numpy as np
import pytest
import torch

import tolerances as T
import tolerances_lse as TL
import test_gpu_kvcache as TK
import test_gpu_kvcache_fp8 as TF
import test_gpu_kvcache_lse as TS

pytestmark = pytest.mark.gpu

DT = TK.DT
H, HK, CAP, PCAP = 8, 2, 160, 208


def _F():
    import flash_cosine_sim_attention_amd as F
    return F


def _rnd(dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float32).to(DT[dtype])


def _materialise(pk, pv, P, kc, vc):
    """[B, Hk, P + cap, D] caches: the first P prefix positions, then each sequence's own cache"""
    B = kc.shape[0]
    return (torch.cat([pk[:, :, :P].expand(B, -1, -1, -1), kc], dim=2).contiguous(),
            torch.cat([pv[:, :, :P].expand(B, -1, -1, -1), vc], dim=2).contiguous())


def _guarded(t):
    """a copy of t inside a NaN arena: (arena, view, guard elements)"""
    guard = 2048
    arena = torch.full((2 * guard + t.numel(),), float("nan"), device=t.device, dtype=t.dtype)
    view = arena[guard:guard + t.numel()].view(t.shape)
    view.copy_(t)
    return arena, view, guard


def check_against_plain(dtype, o, lse, plain, lse_plain, label):
    """The shared-prefix result against the plain call on the materialised caches, at the composed route's own bars (COMPOSED_FWD_TOL:
    excess over one output ulp, rel-L2) and the LSE bar; rows without any key agree exactly."""
    dead = lse_plain == float("-inf")
    assert torch.equal(lse == float("-inf"), dead) and (o[dead] == 0).all() and (plain[dead] == 0).all(), label
    if (~dead).any():
        d = float((lse - lse_plain)[~dead].abs().max())
        assert T.check(label + "/vs-plain-lse", dtype, d, TL.LSE_TOL[dtype]), (label, d)
    atol, rtol, rel = TL.COMPOSED_FWD_TOL[dtype]
    go, gp = TS._np(o), TS._np(plain)
    excess = float((np.abs(go - gp) - rtol * np.abs(gp)).max(initial=0.0))
    assert T.check(label + "/vs-plain-excess", dtype, excess, atol), (label, excess, atol)
    assert T.check(label + "/vs-plain-rel", dtype, TK._rel(go, gp), rel), (label, TK._rel(go, gp), rel)


CASES = [(dtype, D, P, N, causal) for dtype in ("bf16", "f16", "f32") for D in (64, 128) for P in (0, 45, 200) for N in (1, 3)
         for causal in (False, True) if dtype == "bf16" or (D, N) in ((64, 3), (128, 1))]


@pytest.mark.parametrize("dtype,D,P,N,causal", CASES, ids=[f"{c[0]}_d{c[1]}_p{c[2]}_n{c[3]}_{'causal' if c[4] else 'full'}" for c in CASES])
def test_shared_prefix_equal_n(dtype, D, P, N, causal):
    F = _F()
    B, own = 3, [0, 17, 130]
    r = _rnd(dtype, seed=D + P + N)
    q, pk, pv, kc, vc = r(B, H, N, D), r(1, HK, PCAP, D), r(1, HK, PCAP, D), r(B, HK, CAP, D), r(B, HK, CAP, D)
    append = causal                                       # causal: the step's tokens are appended (L_b = own + N); else L_b = own
    kn, vn = (r(B, HK, N, D), r(B, HK, N, D)) if append else (None, None)
    sl = torch.tensor(own, dtype=torch.int32, device="cuda")
    lens = [n + (N if append else 0) for n in own]
    (arena_pk, pk_g, guard), (arena_pv, pv_g, _) = _guarded(pk), _guarded(pv)
    fk, fv = _materialise(pk, pv, P, kc, vc)
    kc_s, vc_s, kc_f, vc_f = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    with torch.no_grad():
        o, lse = F.flash_cosine_sim_attention_with_shared_prefix(q, pk_g, pv_g, kc, vc, prefix_len=P, k_new=kn, v_new=vn, cache_seqlens=sl,
                                                                  causal=causal, return_lse=True)
        o_only = F.flash_cosine_sim_attention_with_shared_prefix(q, pk_g, pv_g, kc_f, vc_f, prefix_len=P, k_new=kn, v_new=vn, cache_seqlens=sl,
                                                                 causal=causal)
        plain, lse_plain = F.flash_cosine_sim_attention_with_kvcache(q, fk, fv, kn, vn, sl + P, causal=causal, return_lse=True)
        suffix, lse_suffix = F.flash_cosine_sim_attention_with_kvcache(q, kc_s, vc_s, kn, vn, sl, causal=causal, return_lse=True)
    torch.cuda.synchronize()
    assert TS.TK_bits_equal(o, o_only)
    # the append lands in the own caches only (exactly the suffix call's append); the prefix and its surroundings keep their bits
    assert TS.TK_bits_equal(kc, kc_s) and TS.TK_bits_equal(vc, vc_s)
    assert TS.TK_bits_equal(pk_g, pk) and TS.TK_bits_equal(pv_g, pv)
    for arena in (arena_pk, arena_pv):
        assert torch.isnan(arena[:guard]).all() and torch.isnan(arena[-guard:]).all()
    if P == 0:
        assert TS.TK_bits_equal(o, suffix) and TS.TK_bits_equal(lse, lse_suffix)
    label = f"prefix_{dtype}_d{D}_p{P}_n{N}_{'causal' if causal else 'full'}"
    ks, vs = TK._seqs(fk, fv, [P + L for L in lens])
    TS.check_composed(dtype, o, q, ks, vs, dict(causal=causal), label)
    TS.check_lse(dtype, lse, q, ks, dict(causal=causal), label)
    check_against_plain(dtype, o, lse, plain, lse_plain, label)


# the same cases through cu_seqlens_q: every D x P x causal for bf16, the other types on one D each
RAGGED = [(dtype, D, P, causal) for dtype in ("bf16", "f16", "f32") for D in (64, 128) for P in (0, 45, 200) for causal in (False, True)
          if dtype == "bf16" or D == {"f16": 64, "f32": 128}[dtype]]


@pytest.mark.parametrize("dtype,D,P,causal", RAGGED, ids=[f"{c[0]}_d{c[1]}_p{c[2]}_{'causal' if c[3] else 'full'}" for c in RAGGED])
def test_shared_prefix_ragged(dtype, D, P, causal):
    F = _F()
    counts, own = [1, 0, 4, 17], [0, 17, 130, 40]
    B, total = len(counts), sum(counts)
    r = _rnd(dtype, seed=D + P + 1)
    q, pk, pv, kc, vc = r(total, H, D), r(1, HK, PCAP, D), r(1, HK, PCAP, D), r(B, HK, CAP, D), r(B, HK, CAP, D)
    append = causal                                       # as in the equal-N cases: causal steps append their tokens, the others do not
    kn, vn = (r(total, HK, D), r(total, HK, D)) if append else (None, None)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device="cuda")
    sl = torch.tensor(own, dtype=torch.int32, device="cuda")
    fk, fv = _materialise(pk, pv, P, kc, vc)
    kc_s, vc_s = kc.clone(), vc.clone()
    with torch.no_grad():
        o, lse = F.flash_cosine_sim_attention_with_shared_prefix(q, pk, pv, kc, vc, prefix_len=torch.tensor([P], dtype=torch.int32, device="cuda"),
                                                                  cu_seqlens_q=cu, k_new=kn, v_new=vn, cache_seqlens=sl, causal=causal, return_lse=True)
        plain, lse_plain = F.flash_cosine_sim_attention_varlen_with_kvcache(q, fk, fv, cu, kn, vn, sl + P, causal=causal, return_lse=True)
        suffix, lse_suffix = F.flash_cosine_sim_attention_varlen_with_kvcache(q, kc_s, vc_s, cu, kn, vn, sl, causal=causal, return_lse=True)
    torch.cuda.synchronize()
    assert o.shape == q.shape and lse.shape == (total, H)
    assert TS.TK_bits_equal(kc, kc_s) and TS.TK_bits_equal(vc, vc_s)
    if P == 0:          # (a device prefix_len of 0 goes through the merge: the empty prefix state leaves the suffix state's bits)
        assert TS.TK_bits_equal(o, suffix) and TS.TK_bits_equal(lse, lse_suffix)
    lens = [P + n + (c if append else 0) for n, c in zip(own, counts)]
    ks, vs = TK._seqs(fk, fv, lens)
    c = cu.tolist()
    label = f"prefix_ragged_{dtype}_d{D}_p{P}_{'causal' if causal else 'full'}"
    for b in range(B):
        if counts[b] == 0:
            continue
        rows = lambda t: t[c[b]:c[b + 1]].transpose(0, 1).unsqueeze(0)
        if lens[b] > 0:
            TS.check_composed(dtype, rows(o), rows(q), [ks[b]], [vs[b]], dict(causal=causal), f"{label}_seq{b}")
        TS.check_lse(dtype, rows(lse.unsqueeze(-1)).squeeze(-1), rows(q), [ks[b]], dict(causal=causal), f"{label}_seq{b}")
    check_against_plain(dtype, o, lse, plain, lse_plain, label)


def test_shared_prefix_and_sequences_in_one_paged_pool():
    F = _F()
    dtype, D, N, B, page, P = "bf16", 64, 2, 3, 16, 45
    own = [0, 17, 100]
    r = _rnd(dtype, seed=5)
    pmb, mb = 3, 8                                                           # prefix pages, pages per sequence
    nb = pmb + B * mb + 4
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(9)).to(torch.int32)
    ptab, tab = perm[:pmb].reshape(1, pmb).cuda(), perm[pmb:pmb + B * mb].reshape(B, mb).cuda()
    kpool, vpool = r(nb, HK, page, D), r(nb, HK, page, D)
    q, kn, vn = r(B, H, N, D), r(B, HK, N, D), r(B, HK, N, D)
    sl = torch.tensor(own, dtype=torch.int32, device="cuda")
    gather = lambda pool, t: torch.cat([pool[int(i)] for i in t], dim=1)      # [Hk, pages * page, D]
    pk, pv = gather(kpool, ptab[0])[None], gather(vpool, ptab[0])[None]
    kc = torch.stack([gather(kpool, tab[b]) for b in range(B)])
    vc = torch.stack([gather(vpool, tab[b]) for b in range(B)])
    fk, fv = _materialise(pk, pv, P, kc, vc)
    before_k = kpool.clone()
    with torch.no_grad():
        o, lse = F.flash_cosine_sim_attention_with_shared_prefix(q, kpool, vpool, kpool, vpool, prefix_len=P, prefix_block_table=ptab, k_new=kn,
                                                                  v_new=vn, cache_seqlens=sl, block_table=tab, causal=True, return_lse=True)
        plain, lse_plain = F.flash_cosine_sim_attention_with_kvcache(q, fk, fv, kn, vn, sl + P, causal=True, return_lse=True)
    torch.cuda.synchronize()
    # only the appended slots of the sequences' own pages changed
    changed = (kpool != before_k).flatten(1).any(dim=1).nonzero().flatten().tolist()
    assert set(changed) <= {int(tab[b, (own[b] + t) // page]) for b in range(B) for t in range(N)}
    assert not set(changed) & set(ptab.flatten().tolist())
    ks, vs = TK._seqs(fk, fv, [P + n + N for n in own])
    TS.check_composed(dtype, o, q, ks, vs, dict(causal=True), "prefix_paged")
    TS.check_lse(dtype, lse, q, ks, dict(causal=True), "prefix_paged")
    check_against_plain(dtype, o, lse, plain, lse_plain, "prefix_paged")


def test_shared_prefix_fp8():
    F = _F()
    dtype, D, N, B, P = "f16", 64, 1, 3, 200
    own = [0, 17, 130]
    r = _rnd(dtype, seed=6)
    q, pk, pv, kc, vc = r(B, H, N, D), r(1, HK, PCAP, D), r(1, HK, PCAP, D), r(B, HK, CAP, D), r(B, HK, CAP, D)
    (pk8, pks), (pv8, pvs) = TF._quantise(pk), TF._quantise(pv)
    (k8, ks), (v8, vs) = TF._quantise(kc), TF._quantise(vc)
    sl = torch.tensor(own, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        o, lse = F.flash_cosine_sim_attention_with_shared_prefix(q, pk8, pv8, k8, v8, prefix_len=P, cache_seqlens=sl, k_scale=ks, v_scale=vs,
                                                                  prefix_k_scale=pks[0], prefix_v_scale=pvs[0], return_lse=True)
    torch.cuda.synchronize()
    # the values the codes mean, prefix in front: float64 [Hk, P + L_b, D] per sequence
    pkq, pvq = TF._seqs(pk8, pv8, pks, pvs, [P])
    kq, vq = TF._seqs(k8, v8, ks, vs, own)
    kseq = [torch.cat([pkq[0], k], dim=1).cpu().numpy() for k in kq]
    vseq = [torch.cat([pvq[0], v], dim=1).cpu().numpy() for v in vq]
    as_t = lambda xs: [torch.from_numpy(x) for x in xs]
    TS.check_composed(dtype, o, q, as_t(kseq), as_t(vseq), {}, "prefix_fp8")
    TS.check_lse(dtype, lse, q, kseq, {}, "prefix_fp8")


def test_shared_prefix_graph_capture_and_replay():
    F = _F()
    f = F.flash_cosine_sim_attention_with_shared_prefix
    dtype, D, N, B = "bf16", 64, 1, 3
    r = _rnd(dtype, seed=8)
    q, pk, pv, kc, vc = r(B, H, N, D), r(1, HK, PCAP, D), r(1, HK, PCAP, D), r(B, HK, CAP, D), r(B, HK, CAP, D)
    kn, vn = r(B, HK, N, D), r(B, HK, N, D)
    sl = torch.tensor([0, 17, 130], dtype=torch.int32, device="cuda")
    plen = torch.tensor([45], dtype=torch.int32, device="cuda")
    call = lambda kc_, vc_: f(q, pk, pv, kc_, vc_, prefix_len=plen, k_new=kn, v_new=vn, cache_seqlens=sl, max_seqlen_k=CAP, causal=True,
                              return_lse=True)
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            call(kc, vc)                                                      # warm-up (allocator, lazy init)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        kc_eager, vc_eager = kc.clone(), vc.clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out, out_lse = call(kc, vc)
        for step in range(2):
            q.copy_(torch.randn_like(q))
            kn.copy_(torch.randn_like(kn))
            vn.copy_(torch.randn_like(vn))
            sl.copy_(torch.tensor([1 + step, 18 + 2 * step, 131 + step], dtype=torch.int32))
            plen.fill_(46 + 100 * step)
            g.replay()
            ref, ref_lse = call(kc_eager, vc_eager)
            torch.cuda.synchronize()
            assert TS.TK_bits_equal(out, ref) and TS.TK_bits_equal(out_lse, ref_lse), step
            assert torch.equal(kc, kc_eager) and torch.equal(vc, vc_eager), step
