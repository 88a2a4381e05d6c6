"""The visibility probe: inputs on which the softmax is EXACTLY uniform, so that every output is a pure function of the set of visible
(query, key) pairs, and a single hidden or leaked key moves the expected value by more than the bar.  No GPU code here.

Construction ("cone" inputs, l2norm groups = 1).  Feature 0 is the axis:

    q_i = r_i e_0                                  k_j = m_j (e_0 + e_{1 + j % (D - 1)})
    v_j = e_{j % D}                                do_i = e_{i % D}

(Values repeat every D positions and key classes every D - 1: the probe counts keys per class, it is no addressing test -- a block-table
entry that points at another live block of the same sequence at page sizes 16 / 32 and D = 16 / 32 leaves o and lse unchanged; the
random-input and address-range tests cover that.)  r_i, m_j are random powers of two in [1/4, 4]: scaling by them is exact in every dtype.  j is the key's position in its sequence (for a
cache: its cache position, appended keys included), i the query's position in its sequence under the bottom-right alignment every call
uses (row + M - N: the query's diagonal key carries its class, so dS is not identically 0 on rows that see few keys).  q^ = e_0 exactly and both
non-zero features of k^ are the dtype's rounding c of 1/sqrt(2), the same for every key, so every logit of a row is the same number
scale * c whatever the kernel's exponent regime: P is uniform over the row's visible keys in any correct implementation.  With
l2norm_qk=False the rows are supplied normalised (r = m = 1, k = c (e_0 + e_.)).  Then

    o[i, f]   = #{visible j : j % D == f} / cnt_i                       lse_i = logit + ln cnt_i
    dv[j, f]  = sum over the rows i that see j with i % D == f of 1 / cnt_i
    dS[i, j]  = ([i % D == j % D] - delta_i) / cnt_i,  delta_i = o[i, i % D]
    dq^ = scale dS K^,  dk^ = scale dS^T Q^,  through the l2norm backward  dx = (dx^ - x^ <dx^, x^>) / |x|

`expected` evaluates these in float64 over an explicit boolean vis[i, j] for r = m = 1; dq * r_i and dk * m_j of a kernel are compared
with it (exact rescaling), so one expectation serves every batch and head.  A table case with l2norm groups g > 1 is probed with
groups = 1 and scale * g: the bound scale * groups, hence the exponent regime and the kernel form, is the same.

Bars (`check`): elementwise |got - ref| <= bar * mag + tiny.  tiny is the dtype's smallest normal: an element whose every term is 0 must
come out 0.  mag is the sum of the ABSOLUTE values of the terms the element is summed from -- the forward-error bound of a rounded sum.
For o and dv every term is positive and mag = |ref|, the plain relative check.  dq and dk are sums of both signs (dS = P (dP - delta); the
l2norm backward subtracts a projection) and can cancel to exactly 0 (N = M a multiple of D without causal: every dk^ is 0), where a kernel
returns the rounding residue of its 16-bit dS: that rounding is relative to the terms, not to their sum, so mag is carried through the
same formulas with every difference replaced by a sum.  bar: forward, two 16-bit roundings of half an ulp each first order (P~ to the MFMA
operand against the un-rounded row sum, and the output): 2 * eps leaves a factor 2; gradients add the rounding of dS and of the 1/sqrt(2)
operand: 4 * eps.  float32: the rtol of FWD_TOL and GRAD_TOL of tests/tolerances.py.  lse: 4 * eps_f32 * max(1, |lse|) absolute against
logit + ln cnt with the logit taken from the operands the kernels feed the S product: the dtype's rounding of c1 = scale *
log2(e) (q^ = e_0, so c1 q^ is c1) times c, back in natural units; without l2norm_qk scale * c.

The bias probe (`bias_vis`, `BIAS_CASES`, `run_dense_bias`).  attn_bias is -inf where a seeded pattern hides the pair and a per-(slice, row)
integer c[s, i] in -2 .. 2 (exact in every dtype; all 0 on an "offsets" case) where it shows it.  A constant per row leaves the softmax
uniform over vis_eff = pattern & geometry (causal, key mask), so o, dq, dk, dv keep the expectation above -- one `expected` per slice, dk /
dv of a K/V head summed over its group's slices -- while the multiply by log2(e) and both exponent regimes run on finite values and a read
from the wrong row shifts a whole row of weights.  Every slice has its own pattern (30 % random; hidden six-column runs across the 32-,
64-, 128-, 256-key edges and six-row runs across the 32-, 128-, 256-row edges, one visible pair inside, shifting with row / column /
slice), so an off-by-one of any of the three indices changes the visible set.  On these inputs dS does not depend on batch or head:

    d_bias[s, i, j] = R dS_s[i, j],   R = B (per-head bias) or H (per-batch bias),   mag = R P (dP + delta)

and a hidden pair has expectation and mag exactly 0: the kernel must write 0 up to tiny.  Bar of d_bias: the row sum of the rounded P~
(eps / 2), delta from a rounded o (eps / 2 delta) and the one rounding of the store into the bias dtype (eps / 2) are <= 1.5 eps mag to
first order; 4 eps leaves a factor ~2.7 (float32: the rtol of GRAD_TOL).  float16: the smallest non-zero |d_bias| is delta_i / cnt_i,
~3.5e-6 at 1100 keys and below tiny = 6.1e-5, so a float16 case multiplies do by a power of two g (exact; every gradient expectation
scales by it) chosen FROM THE EXPECTATION so that the smallest non-zero |d_bias| is >= 16 tiny.

`decidable`: whether flipping one boundary pair of vis moves the float64 expectation of a quantity by >= 1.5 * bar * mag in some element.
8 significant bits separate about 1 / (1.5 * bar) keys per feature: ~40 D visible keys for o and ~20 (D - 1) for gradients in bf16.
"""
import math

import numpy as np
import torch

import tolerances as T

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
LOG2E = 1.4426950408889634
FLIP_SAMPLE = 256


# ---- bars ------------------------------------------------------------------------------------------------------------------------------------

def eps(dtype):
    return torch.finfo(DT[dtype]).eps


def tiny(dtype):
    return torch.finfo(DT[dtype]).tiny


def bar(dtype, quantity):
    """the relative bar of o / dq / dk / dv / dbias (module docstring)"""
    if dtype == "f32":
        return T.FWD_TOL["f32"][1] if quantity == "o" else T.GRAD_TOL["f32"]
    return (2 if quantity == "o" else 4) * eps(dtype)


def rounded(x, dtype):
    """x rounded to the dtype (round to nearest even), as a Python float"""
    return float(torch.tensor(float(x), dtype=torch.float64).to(DT[dtype]).double())


def cone(dtype):
    """the dtype's 1 / sqrt(2): both non-zero features of every normalised key"""
    return rounded(1.0 / math.sqrt(2.0), dtype)


def logit(dtype, scale, l2norm_qk=True):
    """every visible pair's logit in natural units, from the operands of the S product"""
    if not l2norm_qk:
        return scale * cone(dtype)
    c1 = float(np.float32(scale) * np.float32(LOG2E))
    return rounded(c1, dtype) * cone(dtype) / LOG2E


# ---- visibility builders: one per feature, from the docstrings of ops.py ------------------------------------------------------------------

def vis_mask(N, mask):
    """key mask: every query sees key j iff mask[j]"""
    return np.broadcast_to(np.asarray(mask, bool)[None, :], (N, len(mask))).copy()


def vis_causal(N, M):
    """bottom-right aligned: key j is visible to query i iff j - (M - N) <= i"""
    return np.arange(M)[None, :] - (M - N) <= np.arange(N)[:, None]


def vis_window(N, M, left, right):
    """i + (M - N) - left <= j <= i + (M - N) + right; -1: unbounded side"""
    t = np.arange(N)[:, None] + (M - N)
    j = np.arange(M)[None, :]
    vis = np.ones((N, M), bool)
    if left >= 0:
        vis &= j >= t - left
    if right >= 0:
        vis &= j <= t + right
    return vis


def vis_dense(N, M, causal=False, window=(-1, -1), mask=None):
    """one dense problem: the window, under causal also the causal cut (which is what capping the window's right side at 0 means), the mask"""
    vis = vis_window(N, M, window[0], window[1])
    if causal:
        vis = vis & vis_causal(N, M)
    return vis if mask is None else vis & vis_mask(N, mask)


def vis_spans(lens_q, lens_k, causal=False, window=(-1, -1)):
    """a packed batch: sequence s is the dense problem (N_s, M_s) on its own"""
    return [vis_dense(n, m, causal, window) for n, m in zip(lens_q, lens_k)]


def vis_cache(N, cached, n_new, causal=False, window=(-1, -1), capacity=None):
    """a cache call: L = cached + n_new positions (slots at or beyond the capacity are dropped), the N queries the last N of them"""
    L = cached + n_new if capacity is None else min(cached + n_new, capacity)
    return vis_dense(N, L, causal, window)


def vis_ragged(counts, cached, append, causal=False, window=(-1, -1)):
    """a ragged decode step: sequence b has N_b queries against L_b = cached_b (+ N_b with an append)"""
    return [vis_cache(n, c, n if append else 0, causal, window) for n, c in zip(counts, cached)]


def vis_shared_prefix(P, own):
    """the P prefix positions (visible to every query), then the sequence's own positions"""
    return np.concatenate([np.ones((own.shape[0], P), bool), own], axis=1)


# ---- the float64 expectation ---------------------------------------------------------------------------------------------------------------

def _khat(kpos, D, c):
    K = np.zeros((len(kpos), D))
    K[:, 0] = c
    K[np.arange(len(kpos)), 1 + kpos % (D - 1)] = c
    return K


def _l2_backward(g, mag, xhat, norm):
    """dx = (g - x^ <g, x^>) / |x| and its sum-of-absolute-terms companion"""
    dx = (g - xhat * (g * xhat).sum(-1, keepdims=True)) / norm
    m = (mag + np.abs(xhat) * (mag * np.abs(xhat)).sum(-1, keepdims=True)) / norm
    return dx, m


def expected(vis, D, dtype, scale=8.0, l2norm_qk=True, kpos=None, grads=True, qpos=None):
    """float64 attention over vis[i, j] on the cone inputs with r = m = 1.  kpos: the keys' positions (default 0 .. M - 1; a shared prefix
    passes prefix positions followed by own positions); qpos: the queries' positions (default i + M - N, the bottom-right alignment: the
    query's diagonal key carries its class).  Returns a dict: o [N, D], lse [N]; with grads dq [N, D], dk, dv [M, D] of ONE query
    head (dk, dv of a K/V head are the sum over its query group: G times these), ds [N, M] (dS = P (dP - delta): what one (batch, head) adds
    to d_bias) and mag_* for every quantity.  Rows without a visible key give o = 0, lse = -inf and contribute no gradient."""
    vis = np.asarray(vis, bool)
    N, M = vis.shape
    kpos = np.arange(M) if kpos is None else np.asarray(kpos)
    c = cone(dtype)
    cnt = vis.sum(1)
    inv = np.where(cnt > 0, 1.0 / np.maximum(cnt, 1), 0.0)
    V = np.zeros((M, D), np.float32)
    V[np.arange(M), kpos % D] = 1.0
    o = (vis.astype(np.float32) @ V).astype(np.float64) * inv[:, None]      # (counts: exact in float32; no N x M float64 matrix for forward-only cases)
    with np.errstate(divide="ignore"):
        lse = np.where(cnt > 0, logit(dtype, scale, l2norm_qk) + np.log(np.maximum(cnt, 1)), -np.inf)
    out = dict(o=o, mag_o=o, lse=lse, cnt=cnt)
    if not grads:
        return out
    P = vis * inv[:, None]
    qcls = (np.arange(N) + (M - N) if qpos is None else np.asarray(qpos)) % D
    dO = np.zeros((N, D))
    dO[np.arange(N), qcls] = 1.0
    dP = (qcls[:, None] == (kpos % D)[None, :]).astype(np.float64)
    delta = o[np.arange(N), qcls]
    dS, magS = P * (dP - delta[:, None]), P * (dP + delta[:, None])
    dv = P.T @ dO
    K = _khat(kpos, D, c)
    Q = np.zeros((N, D))
    Q[:, 0] = 1.0
    dq, mag_dq = scale * dS @ K, abs(scale) * magS @ K
    dk, mag_dk = scale * dS.T @ Q, abs(scale) * magS.T @ Q
    if l2norm_qk:
        dq, mag_dq = _l2_backward(dq, mag_dq, Q, 1.0)
        dk, mag_dk = _l2_backward(dk, mag_dk, K, math.sqrt(2.0))
    out.update(dq=dq, mag_dq=mag_dq, dk=dk, mag_dk=mag_dk, dv=dv, mag_dv=dv, ds=dS, mag_ds=magS)
    return out


def expected_autograd(vis, D, dtype, scale=8.0, l2norm_qk=True, bias=None):
    """the same o, dq, dk, dv from torch float64 autograd through the l2norm: the closed form's cross-check (CPU test).  bias [N, M]
    (0 / c_i / -inf): added to the logits as a leaf before the fill of vis (the geometry); its gradient comes back as d_bias"""
    vis = torch.as_tensor(np.asarray(vis, bool))
    N, M = vis.shape
    c = cone(dtype)
    q = torch.zeros(N, D, dtype=torch.float64)
    q[:, 0] = 1.0
    k = torch.as_tensor(_khat(np.arange(M), D, 1.0 if l2norm_qk else c))
    v = torch.zeros(M, D, dtype=torch.float64)
    v[torch.arange(M), torch.arange(M) % D] = 1.0
    do = torch.zeros(N, D, dtype=torch.float64)
    do[torch.arange(N), (torch.arange(N) + (M - N)) % D] = 1.0
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    # the normalised keys are c (e_0 + e_.) with the ROUNDED c: the l2norm's Jacobian at the unit vector, times c sqrt(2)
    qh, kh = (q / q.norm(dim=-1, keepdim=True), k / k.norm(dim=-1, keepdim=True) * (c * math.sqrt(2.0))) if l2norm_qk else (q, k)
    s = scale * qh @ kh.T
    if bias is not None:
        bias = torch.as_tensor(np.asarray(bias, np.float64)).requires_grad_()
        s = s + bias
    s = s.masked_fill(~vis, float("-inf"))
    some = torch.isfinite(s).any(1, keepdim=True)
    p = torch.where(some, torch.softmax(torch.where(some, s, torch.zeros_like(s)), -1), torch.zeros_like(s))
    o = p @ v
    o.backward(do)
    out = dict(o=o.detach().numpy(), dq=q.grad.numpy(), dk=k.grad.numpy(), dv=v.grad.numpy())
    if bias is not None:
        out["d_bias"] = bias.grad.numpy()
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------

def _pow2(gen, shape, on):
    return torch.exp2(torch.randint(-2, 3, shape, generator=gen).double()) if on else torch.ones(shape, dtype=torch.float64)


def probe_queries(dtype, lead, N, D, l2norm_qk=True, seed=0, first=0):
    """q [*lead, N, D] = r e_0 and do = e_{(first + i) % D} (first: the position of query 0, M - N under the bottom-right alignment), with
    r [*lead, N] (float64, CPU)"""
    gen = torch.Generator().manual_seed(seed)
    r = _pow2(gen, (*lead, N), l2norm_qk)
    q = torch.zeros(*lead, N, D, dtype=torch.float64)
    q[..., 0] = r
    do = torch.zeros(*lead, N, D, dtype=torch.float64)
    do[..., torch.arange(N), (torch.arange(N) + first) % D] = 1.0
    return q.to(DT[dtype]), do.to(DT[dtype]), r


def probe_keys(dtype, lead, M, D, l2norm_qk=True, seed=1, pos=None):
    """k [*lead, M, D] = m (e_0 + e_{1 + j % (D - 1)}) (normalised and rounded without l2norm_qk), v = e_{j % D}, with m [*lead, M]"""
    gen = torch.Generator().manual_seed(seed)
    m = _pow2(gen, (*lead, M), l2norm_qk)
    pos = torch.arange(M) if pos is None else torch.as_tensor(pos)
    k = torch.zeros(*lead, M, D, dtype=torch.float64)
    k[..., 0] = m
    k[..., torch.arange(M), 1 + pos % (D - 1)] = m
    if not l2norm_qk:
        k = k * cone(dtype)
    v = torch.zeros(*lead, M, D, dtype=torch.float64)
    v[..., torch.arange(M), pos % D] = 1.0
    return k.to(DT[dtype]), v.to(DT[dtype]), m


def probe_inputs(dtype, B, H, Hk, N, M, D, l2norm_qk=True, seed=0):
    """the dense probe: q, do [B, H, N, D], k, v [B, Hk, M, D] and the scalings r [B, H, N], m [B, Hk, M]"""
    q, do, r = probe_queries(dtype, (B, H), N, D, l2norm_qk, seed, first=M - N)
    k, v, m = probe_keys(dtype, (B, Hk), M, D, l2norm_qk, seed + 1)
    return q, k, v, do, r, m


def probe_scale(kw):
    """(scale, l2norm_qk) of the probe's copy of a table case: groups = 1 and scale * groups (same bound, same regime and form)"""
    return float(kw.get("scale", 8.0)) * kw.get("groups", 1), kw.get("l2norm_qk", True)


# ---- comparison -------------------------------------------------------------------------------------------------------------------------------

def ratio(dtype, got, ref, mag):
    """max over the elements of (|got - ref| - tiny) / mag: the figure held against the bar; inf where an element without any term is not
    0 up to tiny (or anything is not finite).  got: a tensor or array broadcastable against ref / mag."""
    got = torch.as_tensor(got).detach().double()
    ref, mag = (torch.as_tensor(np.ascontiguousarray(x)).to(got.device) for x in (ref, mag))
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return math.inf
    over = ((got - ref).abs() - tiny(dtype)).clamp_min(0.0)
    mag = mag.expand_as(over)
    worst = torch.where(mag > 0, over / mag.clamp_min(1e-300), torch.where(over > 0, torch.full_like(over, math.inf), torch.zeros_like(over)))
    return float(worst.max())


def check(dtype, got, ref, label, quantity="o", mag=None, case=None):
    """the elementwise check of the module docstring, through tolerances.check (FCSA_TOL_LOG records it); returns (ok, measured, bar)"""
    measured = ratio(dtype, got, ref, np.abs(ref) if mag is None else mag)
    b = bar(dtype, quantity)
    return T.check(f"probe/{quantity}/{label}", dtype, measured, b, case), measured, b


def check_lse(dtype, got, ref, label, case=None):
    """-inf exactly where the expectation is, elsewhere |got - ref| <= 4 eps_f32 max(1, |ref|); returns (ok, measured ratio, 1.0)"""
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(np.ascontiguousarray(ref)).expand_as(got)
    dead = torch.isinf(ref)
    if not torch.equal(torch.isneginf(got), dead) or bool(torch.isnan(got).any()):
        measured = math.inf
    else:
        allow = 4 * torch.finfo(torch.float32).eps * ref[~dead].abs().clamp_min(1.0)
        measured = float(((got[~dead] - ref[~dead]).abs() / allow).max()) if allow.numel() else 0.0
    return T.check(f"probe/lse/{label}", dtype, measured, 1.0, case), measured, 1.0


# ---- decidability ---------------------------------------------------------------------------------------------------------------------------

def boundary_flips(vis, seed=0):
    """every visible pair next to a hidden one and every hidden pair next to a visible one (neighbours along the row and along the column);
    all of them up to 256, else a seeded sample of 256"""
    vis = np.asarray(vis, bool)
    edge = np.zeros_like(vis)
    edge[:, 1:] |= vis[:, 1:] != vis[:, :-1]
    edge[:, :-1] |= vis[:, 1:] != vis[:, :-1]
    edge[1:, :] |= vis[1:, :] != vis[:-1, :]
    edge[:-1, :] |= vis[1:, :] != vis[:-1, :]
    flips = np.argwhere(edge)
    if len(flips) > FLIP_SAMPLE:
        flips = flips[np.sort(np.random.default_rng(seed).choice(len(flips), FLIP_SAMPLE, replace=False))]
    return [(int(i), int(j)) for i, j in flips]


def _row(visrow, f, D, c, scale, l2norm_qk, kcls, vcls):
    """o, dq, mag_dq and P of ONE query row (the row-local part of `expected`)"""
    cnt = int(visrow.sum())
    if cnt == 0:
        z = np.zeros(D)
        return z, z, z, np.zeros(len(visrow))
    p = visrow / cnt
    o = np.bincount(vcls[visrow], minlength=D) / cnt
    same = (vcls == f) & visrow
    ds, ms = p * (same - o[f]), p * (same + o[f])
    dq, mq = np.zeros(D), np.zeros(D)
    dq[0], mq[0] = ds.sum(), ms.sum()
    dq[1:] = np.bincount(kcls[visrow] - 1, weights=ds[visrow], minlength=D - 1)
    mq[1:] = np.bincount(kcls[visrow] - 1, weights=ms[visrow], minlength=D - 1)
    dq, mq = scale * c * dq, abs(scale) * c * mq
    if l2norm_qk:
        mq[0] *= 2.0
        dq[0] = 0.0
    return o, dq, mq, p


def decidable(vis, dtype, quantity, D, scale=8.0, l2norm_qk=True, kpos=None, seed=0):
    """True iff EVERY sampled boundary flip of vis moves the float64 expectation of `quantity` (o, dq or dv) by at least 1.5 * bar * mag in
    at least one element.  A flip changes one row of P: o and dq move in that row, dv in that row's feature of every key the row sees.
    dq of a row with at most one visible key is 0 whatever q, k, v and do are (a softmax over one key has no derivative), so a flip
    between no key and one key is outside what dq can decide on ANY input: dq's sample leaves those out (o and dv decide them)."""
    vis = np.asarray(vis, bool)
    N, M = vis.shape
    kpos = np.arange(M) if kpos is None else np.asarray(kpos)
    kcls, vcls, c = 1 + kpos % (D - 1), kpos % D, cone(dtype)
    need = 1.5 * bar(dtype, quantity)
    dv = None
    if quantity == "dv":
        dv = expected(vis, D, dtype, scale, l2norm_qk, kpos)["dv"]
    for i, j in boundary_flips(vis, seed):
        row, f = vis[i].copy(), (i + M - N) % D
        if quantity == "dq" and row.sum() + (not row[j]) <= 1:
            continue
        o0, dq0, mq0, p0 = _row(row, f, D, c, scale, l2norm_qk, kcls, vcls)
        row[j] = not row[j]
        o1, dq1, mq1, p1 = _row(row, f, D, c, scale, l2norm_qk, kcls, vcls)
        if quantity == "o":
            moved = np.abs(o1 - o0) >= need * o0 + tiny(dtype)
        elif quantity == "dq":
            moved = np.abs(dq1 - dq0) >= need * mq0 + tiny(dtype)
        else:
            moved = np.abs(p1 - p0) >= need * dv[:, f] + tiny(dtype)
            moved &= (p1 != p0)
        if not moved.any():
            return False
    return True


# ---- the probe's own case tables (no torch: plain tuples) ---------------------------------------------------------------------------------
# Dense calls without a window: one case per forward, dQ and dK/dV form fcsa_dispatch.h can choose for a dense problem, each with a key
# mask and with causal at N < M and N > M, lengths of t - 1, t, t + 1 for t = 128 and 256 (test_visibility_probe_cpu.py confirms the forms
# with the launch recorder at 256 CUs).  Grids as in window_cases.py: "full" 224 .. 256 workgroups of 256-row tiles (8-wave and lean forms,
# the wide D = 128 forward), "tail" a last round filled under 55 % (16-bit 4-wave forms), "small" (key-split 8-wave forms, float32 4-wave),
# "split" one long side of 1100 (split-key forward and dQ, split-query dK/dV).
LENGTHS = (127, 128, 129, 255, 256, 257)
# (bf16 at D = 16 separates ~20 (D - 1) = 300 keys in a gradient: below the lengths of this table, so D = 16 runs in float16)
DENSE_TYPES = (("bf16", 64), ("f16", 128), ("f32", 32), ("bf16", 32), ("f16", 96), ("f16", 16))
VARIANTS = ("mask", "causal_n<m", "causal_n>m")


def _dense_shape(grid, variant, i, D=64):
    L = LENGTHS[i % len(LENGTHS)]
    other = LENGTHS[(i + 2) % len(LENGTHS)] + (150 if i % 2 else 0)
    if grid == "split":
        L, other = 257, 1100 + i % 3
    if variant == "mask":
        N, M = (L, other) if i % 2 == 0 or grid == "split" else (other, L)
        if grid == "split" and i % 2:
            N, M = M, N
        elif grid != "split" and M < 2 * D:                 # (key_mask keeps a key of every class: it needs two keys per class to hide one)
            N, M = min(N, M), max(N, M)
    elif variant == "causal_n<m":
        N, M = min(L, other), max(L, other) + (L == other)
    elif variant == "causal_n>m":
        N, M = max(L, other) + (L == other), min(L, other)
    else:                                                  # "plain": no mask, N != M -- only the end of the keys is a boundary
        N, M = L, other
    return N, M


def _dense_cases():
    out, i = [], 0
    for dtype, D in DENSE_TYPES:
        for grid in ("full", "tail", "small", "split"):
            if grid == "split" and D < 64:                 # (1100 keys are beyond what 8 bits separate at D = 16 / 32)
                continue
            for variant in VARIANTS:
                N, M = _dense_shape(grid, variant, i, D)
                causal = variant.startswith("causal")
                # heads by the longer grid side: forward / dQ tile the queries, dK/dV the keys
                pairs = lambda n: ((n + 255) // 256 + 1) // 2 if causal else (n + 255) // 256
                p = max(pairs(N), pairs(M))
                B, H = {"full": (max(1, 8 // p), 30), "tail": (max(1, 10 // p), 30), "small": (1, 8), "split": (1, 8)}[grid]
                Hk = H if grid in ("full", "tail") else (H, 2, 1)[(i + i // 3) % 3]
                out.append((f"{dtype}_d{D}_{grid}_{variant}_n{N}m{M}_h{H}k{Hk}", dtype, D, B, H, Hk, N, M, variant, dict(), 1, 1, True))
                i += 1
    # the D = 128 wide forward (64 rows per wave) and the lean form it replaces: fcsa_debug_forward_form 1 / 0; it takes no key mask
    for dtype in ("f16", "bf16"):
        for ff in (1, 0):
            for variant in ("plain", "causal_n<m", "causal_n>m"):
                N, M = _dense_shape("full", variant, i)
                out.append((f"{dtype}_d128_wide{ff}_{variant}_n{N}m{M}", dtype, 128, 8, 30, 30, N, M, variant, dict(), ff, 1, True))
                i += 1
    # grouped-query K/V: the group sweep (fcsa_debug_kv_group_form 2) and the per-head slabs (0), and the automatic choice
    for dtype, D in (("bf16", 64), ("f16", 128)):
        for kf in (2, 0, 1):
            for variant in VARIANTS:
                N, M = _dense_shape("full", variant, i, D)
                out.append((f"{dtype}_d{D}_gqa_kf{kf}_{variant}_n{N}m{M}", dtype, D, 8, 32, 8, N, M, variant, dict(), 1, kf, True))
                i += 1
    # the split-key forward: few heads over 2100 keys (float32: 1100), float16 / D = 128 so that one key of 2100 still moves 8 .. 11 bits
    for dtype, D, H, Hk, N, M, variant in (("f16", 64, 8, 8, 129, 2100, "mask"), ("f16", 128, 4, 1, 257, 2101, "causal_n<m"),
                                           ("bf16", 128, 2, 2, 127, 2100, "mask"), ("f32", 32, 2, 2, 128, 1100, "mask"),
                                           # the causal split-query dK/dV needs >= 1024 of both sides; the query-split 8-wave form >= 512 rows
                                           ("f16", 128, 2, 2, 1101, 1100, "causal_n>m"), ("f16", 128, 2, 2, 1100, 1101, "causal_n<m"),
                                           ("bf16", 64, 8, 8, 600, 700, "causal_n<m"), ("f16", 128, 2, 2, 2200, 2100, "causal_n>m")):
        out.append((f"{dtype}_d{D}_fsplit_{variant}_n{N}m{M}_h{H}k{Hk}", dtype, D, 1, H, Hk, N, M, variant, dict(), 1, 1, True))
    # the 64-rows-per-wave D = 32 forward (fwd2_kernel: 16-bit, no mask, >= 224 workgroups of 256 rows, from 4096 keys; causal from 8192
    # rows): float16, whose o separates ~340 D = 10900 keys; forward only (no backward kernel is special to these shapes)
    for B, H, N, M, variant in ((4, 30, 257, 4097, "plain"), (8, 30, 255, 4096, "plain"), (1, 14, 8192, 8300, "causal_n<m"),
                                (1, 14, 8300, 8192, "causal_n>m")):
        out.append((f"f16_d32_fwd2_{variant}_n{N}m{M}", "f16", 32, B, H, H, N, M, variant, dict(), 1, 1, False))
    # both shift regimes and inputs already normalised, on small grids
    for dtype, D, kw in (("bf16", 64, dict(scale=80.0)), ("f16", 64, dict(scale=16.0)), ("f32", 64, dict(scale=80.0)),
                         ("bf16", 128, dict(l2norm_qk=False, scale=1.0)), ("f16", 32, dict(l2norm_qk=False, scale=1.0))):
        for variant in VARIANTS:
            N, M = _dense_shape("small", variant, i, D)
            out.append((f"{dtype}_d{D}_{'nol2' if 'l2norm_qk' in kw else 'per_row'}_{variant}_n{N}m{M}", dtype, D, 1, 8, (8, 2, 1)[i % 3], N, M,
                        variant, kw, 1, 1, True))
            i += 1
    return out


# id, dtype, D, B, H, Hk, N, M, variant, kwargs, forward form knob, kv-group form knob, with backward
DENSE_PLAIN_CASES = _dense_cases()


def key_mask(M, seed, D=None):
    """a key mask with structure at every boundary a kernel has: ~30 % of the keys hidden at random, hidden runs across the 32-, 64-, 128-
    and 256-key edges with a single visible key inside, both ends set by the seed.  With D, one key of every value class j % D stays visible
    (a row that sees no key of its own class has dS = 0 on the probe, and dq could not see a flip in it)"""
    rng = np.random.default_rng(seed)
    mask = rng.random(M) > 0.3
    for edge in (32, 64, 128, 256):
        if edge + 3 < M:
            mask[edge - 3:edge + 3] = False
            mask[edge - 1 if seed % 2 else edge] = True
    mask[0], mask[-1] = bool(seed & 1), bool(seed & 2)
    if not mask.any():
        mask[M // 2] = True
    if D is not None:
        for cls in range(min(D, M)):
            if not mask[cls::D].any():
                mask[cls + D * int(rng.integers(len(mask[cls::D])))] = True
    return mask


def dense_plain_vis(case):
    """(vis, mask or None, causal) of a DENSE_PLAIN_CASES entry"""
    name, dtype, D, B, H, Hk, N, M, variant = case[:9]
    if variant == "mask":
        mask = key_mask(M, sum(map(ord, name)), D)
        return vis_dense(N, M, mask=mask), mask, False
    causal = variant.startswith("causal")
    return vis_dense(N, M, causal=causal), None, causal


# ---- the bias probe: attn_bias as a per-(slice, query, key) visibility ---------------------------------------------------------------------

def bias_vis(owners, N, M, D, causal, seed, mask=None):
    """the bias pattern, boolean [owners, N, M] (owners: H for a per-head bias, B for attn_bias_batch_dim=True): True where the bias is
    finite.  Every slice has its own seeded pattern: ~30 % of the pairs hidden at random; hidden runs of six columns across the 32-, 64-,
    128- and 256-key edges with one visible key inside, the run's position shifting with the row (and the slice); the same kind of run
    along the rows across the 32-, 128- and 256-row edges, shifting with the column; the last column and the last row drawn on their own.
    As in key_mask, every row that the geometry (causal, the key mask if any) leaves a key of its own class (i + M - N) % D keeps one
    visible (without it dS of the row is 0 and the row decides nothing)."""
    rng = np.random.default_rng(seed)
    vis = rng.random((owners, N, M)) > 0.3
    rows, cols = np.arange(N), np.arange(M)
    for s in range(owners):
        for edge in (32, 64, 128, 256):
            if edge + 3 < M:
                start = edge - 4 + (rows + s) % 3                       # the run [start, start + 6) crosses the edge for every shift
                for t in range(6):
                    vis[s, rows, start + t] = False
                vis[s, rows, start + 1 + (rows // 3 + s + seed) % 4] = True
        for edge in (32, 128, 256):
            if edge + 3 < N:
                start = edge - 4 + (cols + s) % 3
                for t in range(6):
                    vis[s, start + t, cols] = False
                vis[s, start + 1 + (cols // 3 + s + seed) % 4, cols] = True
        vis[s, :, M - 1] = rng.random(N) > 0.5
        vis[s, N - 1, :] = rng.random(M) > 0.5
    geom = vis_dense(N, M, causal, mask=mask)
    cls = (rows + M - N) % D
    own = geom & (cols[None, :] % D == cls[:, None])                    # the keys of each row's own class that the geometry leaves it
    for s in range(owners):
        for i in np.flatnonzero(own.any(1) & ~(vis[s] & own).any(1)):
            cand = np.flatnonzero(own[i])
            vis[s, i, cand[int(rng.integers(len(cand)))]] = True
    return vis


def bias_rows(owners, N, seed, offsets=False):
    """c[s, i]: the finite bias value of row i of slice s, an integer in -2 .. 2 (exact in every dtype); all 0 on an "offsets" variant"""
    c = np.random.default_rng(seed + 1).integers(-2, 3, (owners, N))
    return np.zeros_like(c) if offsets else c


def bias_values(vis_b, c):
    """the bias as float64 [owners, N, M]: c[s, i] where the pattern shows the pair, -inf where it hides it"""
    return np.where(vis_b, c[:, :, None].astype(np.float64), -np.inf)


def _bias_shape(variant, L, other):
    """(N, M) of a bias case from a tiled length L and the other side: causal variants order them, the others keep L on the query side"""
    if variant == "causal_n<m":
        return min(L, other), max(L, other) + (L == other)
    if variant == "causal_n>m":
        return max(L, other) + (L == other), min(L, other)
    return L, other


# (dQ and dK/dV choose differently for rows <= 128 bytes and wider; bwd_dbias_kernel runs two waves per SIMD up to 128-byte rows, one above)
BIAS_TYPES = (("bf16", 64), ("f16", 128), ("f32", 32), ("bf16", 32), ("f16", 96), ("f16", 16), ("f32", 128))
BIAS_VARIANTS = ("plain", "causal_n<m", "causal_n>m", "mask")
# key lengths of the read and write paths: M % 8 == 0, M % 4 == 0 only, odd (1104 / 1100 / 1101 and 31 / 33 are added by hand below)
BIAS_KEYS = (128, 132, 127, 256, 260, 257, 255, 129)


def _bias_cases():
    """The bias table.  id, dtype, D, B, H, Hk, N, M, variant, kwargs, per-batch bias, offsets variant (all c = 0), misaligned pointer.
    Grids as in _dense_cases: "full" B 8 / H 30 around N 256 (the 8-wave forms), "small" B 1 / H 8 (4-wave and key-split forms), "split"
    257 x ~1100 (the split-key dQ launch) and ~600 x ~300 (the query-split dK/dV); test_visibility_probe_cpu.py holds the launches against
    the bias lines of tests/golden/dispatch_launches.txt.  Every case is decided by o, dv and d_bias; dq is compared at its bar but makes
    no single-pair claim here: among 256 sampled flips of a random two-dimensional pattern some flip almost surely hits a key that shares
    its feature 1 + j % (D - 1) with the row's diagonal key, whose term is cnt times larger (the limit key masks already have).  d_bias
    carries the claim in dq's place: a flipped pair moves it between exactly 0 and a value above 16 tiny."""
    out, i = [], 0

    def add(tag, dtype, D, B, H, Hk, N, M, variant, kw=None, batch=False, offsets=False, misaligned=False):
        name = f"{dtype}_d{D}_{tag}_{variant}_n{N}m{M}_b{B}h{H}k{Hk}" + ("_perbatch" if batch else "") + ("_offsets" if offsets else "") + \
               ("_misaligned" if misaligned else "")
        out.append((name, dtype, D, B, H, Hk, N, M, variant, dict(kw or {}), batch, offsets, misaligned))

    for ti, (dtype, D) in enumerate(BIAS_TYPES):
        for gi, grid in enumerate(("full", "small")):
            for vi, variant in enumerate(BIAS_VARIANTS):
                L, K = LENGTHS[i % len(LENGTHS)], BIAS_KEYS[i % len(BIAS_KEYS)]
                if D >= 64 and (i % 3 == 0 or (variant == "mask" and K < 2 * D)):      # (key_mask needs two keys per class to hide one)
                    K += 148
                N, M = _bias_shape(variant, L, K)
                batch = vi == (ti + 2 * gi) % 4                          # one per-batch bias per dtype and grid, the variant rotating
                B, H = (8, 30) if grid == "full" else (2 if batch else 1, 8)
                Hk = H if grid == "full" else (H, 2, 1)[i % 3]
                add(grid, dtype, D, B, H, Hk, N, M, variant, batch=batch)
                i += 1
    # the split-key dQ launch: few heads, 257 queries against ~1100 keys of each alignment class (no causal: the dispatch gives a problem
    # with a bias no causal split launch at sizes this table allows, and the golden file shows none)
    add("split", "bf16", 64, 1, 8, 8, 257, 1104, "plain")
    add("split", "f16", 128, 1, 8, 2, 257, 1100, "mask")
    add("split", "f32", 32, 2, 8, 8, 257, 1101, "plain", batch=True)
    add("long", "f16", 16, 1, 8, 1, 255, 1100, "plain")
    # the query-split 8-wave dK/dV (N >= 512)
    add("qsplit", "bf16", 64, 1, 8, 8, 601, 300, "plain")
    add("qsplit", "bf16", 64, 1, 8, 2, 600, 257, "mask")
    add("qsplit", "bf16", 64, 1, 8, 8, 521, 700, "causal_n<m")
    add("qsplit", "bf16", 64, 1, 8, 1, 601, 300, "causal_n>m")
    add("qsplit", "f16", 16, 2, 8, 8, 1100, 257, "causal_n>m", batch=True)
    add("qsplit", "bf16", 32, 1, 8, 8, 601, 132, "plain")
    # no whole 32-key block, and one block plus one key (D <= M: every row's class has a key)
    add("small", "f16", 16, 1, 8, 8, 129, 31, "plain")
    add("small", "f16", 16, 1, 8, 2, 127, 33, "mask")
    add("small", "bf16", 32, 1, 8, 8, 30, 33, "causal_n<m")
    add("small", "f32", 32, 2, 8, 8, 129, 33, "causal_n>m", batch=True)
    add("full", "bf16", 32, 8, 30, 30, 255, 33, "plain")
    # a bias whose address is no multiple of 16 bytes, at M % 8 == 0: the scalar read path in every kernel
    add("full", "bf16", 64, 8, 30, 30, 129, 256, "plain", misaligned=True)
    add("small", "f16", 128, 1, 8, 8, 257, 128, "causal_n>m", misaligned=True)
    add("small", "f32", 32, 1, 8, 2, 127, 128, "plain", misaligned=True)
    # the per-row shift in bf16 (scale 80: beyond the constant shift's room), inputs already normalised
    add("per_row", "bf16", 64, 1, 8, 2, 129, 260, "plain", dict(scale=80.0))
    add("per_row", "bf16", 64, 8, 30, 30, 255, 257, "causal_n<m", dict(scale=80.0))
    add("nol2", "bf16", 128, 1, 8, 1, 257, 132, "causal_n>m", dict(l2norm_qk=False, scale=1.0))
    add("nol2", "f16", 32, 1, 8, 8, 127, 256, "mask", dict(l2norm_qk=False, scale=1.0))
    # all finite values 0 (the reference's usual additive mask), next to the default with per-row constants
    for dtype, D, M in (("bf16", 64, 260), ("f16", 128, 257), ("f32", 32, 128)):
        for offsets in (False, True):
            add("pair", dtype, D, 1, 8, 2, 129, M, "plain", offsets=offsets)
    return out


BIAS_CASES = _bias_cases()


# Decode calls without a window.  page 0: contiguous.  lens: cache_seqlens before the append (0, 1, page -+ 1, and capacity - appended);
# counts: None for a rectangular q of N rows, else the per-sequence query counts of a ragged step (appended: every query brings its key).
# id, dtype, D, H, Hk, N, capacity, page, lens, appended keys (rectangular), counts, causal, fp8, kwargs
def _decode_cases():
    out, i = [], 0
    for dtype in ("bf16", "f16", "f32"):
        for N in (1, 5, 17):
            D = (16, 32, 64, 96, 128)[i % 5]
            page, cap = (0, 32, 16)[i % 3], 128
            pg = page or 32
            n_new = (0, 1, N)[(i // 3 + i) % 3]
            lens = [0, 1, pg - 1, pg + 1, cap - n_new]
            causal = i % 2 == 0
            H, Hk = ((4, 4), (8, 2), (4, 1))[i % 3]
            kw = (dict(), dict(scale=16.0 if dtype == "f16" else 80.0), dict(l2norm_qk=False, scale=1.0))[(i // 2) % 3]
            out.append((f"decode_{dtype}_d{D}_n{N}_p{page}_a{n_new}_{'causal' if causal else 'full'}", dtype, D, H, Hk, N, cap, page, lens, n_new,
                        None, causal, False, kw))
            i += 1
    for dtype, D, N, page, n_new, causal in (("bf16", 128, 1, 32, 1, True), ("f16", 64, 5, 0, 5, True), ("bf16", 32, 17, 16, 0, False),
                                            ("f16", 16, 1, 0, 0, False)):
        pg = page or 32
        out.append((f"decode_fp8_{dtype}_d{D}_n{N}_p{page}_a{n_new}", dtype, D, 8, 2, N, 128, page, [0, 1, pg - 1, pg + 1, 128 - n_new], n_new, None,
                    causal, True, dict()))
    # many splits: 2048 keys at D = 128 are 16 keys per feature and up to 16 splits of decode_min_split_keys(128) = 128 keys; the second
    # sequence ends inside a 32-key block
    for dtype in ("bf16", "f16", "f32"):
        out.append((f"decode_{dtype}_d128_splits", dtype, 128, 8, 2, 5, 2048, 0, [2048, 2035], 0, None, True, False, dict()))
    out.append(("decode_fp8_bf16_d128_splits_paged", "bf16", 128, 8, 2, 1, 2048, 64, [2047, 2034], 1, None, False, True, dict()))
    # ragged steps
    for dtype, D, page, append, causal, fp8 in (("bf16", 64, 0, True, True, False), ("f32", 32, 16, False, True, False),
                                               ("f16", 128, 32, True, False, False), ("f16", 96, 0, True, True, True)):
        counts, cached = [1, 0, 5, 17, 3], [0, 31, 33, 100, 1]
        out.append((f"ragged_{'fp8_' if fp8 else ''}{dtype}_d{D}_p{page}_{'append' if append else 'read'}_{'causal' if causal else 'full'}", dtype, D, 8, 2, 0,
                    128, page, cached, 0, counts, causal, fp8, dict(append=append)))
    return out


DECODE_PLAIN_CASES = _decode_cases()

# Shared-prefix steps: prefix lengths 1, page - 1, page + 1 (page 16); rectangular (counts None) and packed; a sequence with N_b = L_b + 1
# (its first query sees the prefix alone under causal).
# id, dtype, D, H, Hk, N, counts, cached (own positions before the append), append, prefix length, prefix paged, causal
PREFIX_CASES = []
for _i, (_dtype, _D) in enumerate((("bf16", 64), ("f16", 128), ("f32", 32), ("bf16", 16))):
    for _j, _P in enumerate((1, 15, 17)):
        _causal = (_i + _j) % 2 == 0
        _paged = (_i + _j) % 3 == 0
        PREFIX_CASES.append((f"prefix_rect_{_dtype}_d{_D}_p{_P}_{'causal' if _causal else 'full'}_append", _dtype, _D, 8, 2, 3, None, [0, 5, 40], True, _P,
                             _paged, _causal))
        PREFIX_CASES.append((f"prefix_rect_{_dtype}_d{_D}_p{_P}_{'causal' if not _causal else 'full'}_first_row_alone", _dtype, _D, 4, 4, 3, None, [2, 2, 2], False,
                             _P, not _paged, not _causal))
        PREFIX_CASES.append((f"prefix_packed_{_dtype}_d{_D}_p{_P}_{'causal' if _causal else 'full'}", _dtype, _D, 8, 2, 0, [1, 4, 0, 3], [0, 3, 9, 20], _j == 1, _P,
                             _paged, _causal))


# ---- running a case: the public call on the probe's inputs, and the comparisons it owes ----------------------------------------------------
# Each runner returns a list of (quantity, label, got, ref, mag): `judge` holds every one against its bar.  device "cpu" runs the package's
# forward-only path (test_visibility_probe_cpu.py, float32), "cuda" the kernels (test_gpu_visibility_probe.py).

def _F():
    import flash_cosine_sim_attention_amd as F
    return F


def judge(dtype, name, comparisons):
    """every comparison printed and logged before the case is judged; returns the failures"""
    fails = []
    for quantity, label, got, ref, mag in comparisons:
        ok, measured, b = check_lse(dtype, got, ref, label, name) if quantity == "lse" else check(dtype, got, ref, label, quantity, mag, name)
        print(f"{name} {label} {quantity}: {measured:.3e} (bar {b:.3e})")
        if not ok:
            fails.append((label, quantity, measured, b))
    return fails


def run_dense(dtype, D, B, H, Hk, N, M, scale, l2norm_qk, device, causal=False, window=None, mask=None, seed=0, grads=True):
    """flash_cosine_sim_attention (window None) or flash_cosine_sim_attention_local on the dense probe"""
    F = _F()
    q, k, v, do, r, m = probe_inputs(dtype, B, H, Hk, N, M, D, l2norm_qk, seed)
    q, k, v, do = (t.to(device) for t in (q, k, v, do))
    if grads:
        q, k, v = (t.requires_grad_() for t in (q, k, v))
    kw = dict(scale=scale, causal=causal, l2norm_qk=l2norm_qk)
    if window is None:
        mask_t = None if mask is None else torch.as_tensor(mask).to(device).expand(B, M).contiguous()
        o = F.flash_cosine_sim_attention(q, k, v, mask=mask_t, **kw)
    else:
        o = F.flash_cosine_sim_attention_local(q, k, v, tuple(window), **kw)
    e = expected(vis_dense(N, M, causal, window or (-1, -1), mask), D, dtype, scale, l2norm_qk, grads=grads)
    out = [("o", "dense", o.detach(), e["o"], e["mag_o"])]
    if grads:
        o.backward(do)
        G = H // Hk
        out += [("dq", "dense", q.grad * r.to(device)[..., None], e["dq"], e["mag_dq"]),
                ("dk", "dense", k.grad * m.to(device)[..., None], G * e["dk"], G * e["mag_dk"]),
                ("dv", "dense", v.grad, G * e["dv"], G * e["mag_dv"])]
    return out


def bias_case_vis(case):
    """(effective visibility [owners, N, M], pattern [owners, N, M], geometry [N, M], key mask or None, causal) of a BIAS_CASES entry"""
    name, dtype, D, B, H, Hk, N, M, variant, kw, batch = case[:11]
    seed = sum(map(ord, name))
    causal = variant.startswith("causal")
    mask = key_mask(M, seed, D) if variant == "mask" else None
    geom = vis_dense(N, M, causal, mask=mask)
    pattern = bias_vis(B if batch else H, N, M, D, causal, seed, mask)
    return pattern & geom[None], pattern, geom, mask, causal


def bias_expected(case, vis_eff=None, g=None):
    """the float64 expectation of a BIAS_CASES entry from one `expected` per slice: o, dq [owners, N, D]; dk, dv [Hk, M, D] (per-head
    bias: the sum over the query heads of the group of their slices) or [B, M, D] (per-batch bias: G times the slice); d_bias [owners, N,
    M] = R dS_s with R the size of the reduced index (B for a per-head bias, H for a per-batch one); mag_* likewise.  "g": the power of two
    float16 cases multiply do by (every gradient expectation here is already multiplied by it) so that the smallest non-zero |d_bias| is at
    least 16 tiny -- computed from the expectation alone (or given: the teeth tests hold a mutated pattern to the factor of the right one); 1
    in the other dtypes, whose tiny is ~1e-38."""
    name, dtype, D, B, H, Hk, N, M, variant, kw, batch = case[:11]
    scale, l2 = probe_scale(kw)
    if vis_eff is None:
        vis_eff = bias_case_vis(case)[0]
    per = [expected(v, D, dtype, scale, l2) for v in vis_eff]
    st = lambda key: np.stack([e[key] for e in per])
    R, G = (H if batch else B), H // Hk
    out = dict(o=st("o"), mag_o=st("mag_o"), dq=st("dq"), mag_dq=st("mag_dq"), d_bias=R * st("ds"), mag_d_bias=R * st("mag_ds"))
    for key in ("dk", "mag_dk", "dv", "mag_dv"):
        x = st(key)
        out[key] = G * x if batch else x.reshape(Hk, G, M, D).sum(1)
    nz = np.abs(out["d_bias"][out["d_bias"] != 0])
    if g is None:
        g = 2.0 ** max(0, math.ceil(math.log2(16 * tiny(dtype) / nz.min()))) if dtype == "f16" and nz.size else 1.0
    for key in list(out):
        if key not in ("o", "mag_o"):
            out[key] = out[key] * g
    out["g"] = g
    return out


def bias_tensor(case, pattern, device="cpu", grads=True):
    """the bias of a case in its dtype, a leaf (grads: requiring grad): -inf / c[s, i]; a misaligned case makes it a contiguous view one element into a larger
    buffer, so that its address is no multiple of 16 bytes (the kernels' vector paths must not be taken)"""
    name, dtype = case[:2]
    offsets, misaligned = case[11:13]
    owners, N, M = pattern.shape
    vals = torch.as_tensor(bias_values(pattern, bias_rows(owners, N, sum(map(ord, name)), offsets))).to(DT[dtype])
    if not misaligned:
        return vals.to(device).requires_grad_(grads)
    buf = torch.zeros(owners * N * M + 8, dtype=DT[dtype], device=device)
    view = buf[1:1 + owners * N * M].view(owners, N, M)
    view.copy_(vals)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view.detach().requires_grad_(grads)


def run_dense_bias(case, device, grads=True):
    """flash_cosine_sim_attention with attn_bias on the dense probe: (comparisons o, dq, dk, dv, d_bias; the bias leaf; the geometry's
    visibility [N, M]).  device "cpu": the forward-only path (grads=False)"""
    F = _F()
    name, dtype, D, B, H, Hk, N, M, variant, kw, batch = case[:11]
    scale, l2 = probe_scale(kw)
    vis_eff, pattern, geom, mask, causal = bias_case_vis(case)
    e = bias_expected(case, vis_eff)
    q, k, v, do, r, m = probe_inputs(dtype, B, H, Hk, N, M, D, l2, len(name))
    q, k, v, do = (t.to(device) for t in (q, k, v, do * e["g"]))
    bias = bias_tensor(case, pattern, device, grads)
    if grads:
        q, k, v = (t.requires_grad_() for t in (q, k, v))
    mask_t = None if mask is None else torch.as_tensor(mask).to(device).expand(B, M).contiguous()
    o = F.flash_cosine_sim_attention(q, k, v, mask=mask_t, attn_bias=bias, attn_bias_batch_dim=batch, scale=scale, causal=causal, l2norm_qk=l2)
    lead = (lambda x: x[:, None]) if batch else (lambda x: x[None])                       # a slice per batch element / per head
    out = [("o", "bias", o.detach(), lead(e["o"]), lead(e["mag_o"]))]
    if grads:
        o.backward(do)
        out += [("dq", "bias", q.grad * r.to(device)[..., None], lead(e["dq"]), lead(e["mag_dq"])),
                ("dk", "bias", k.grad * m.to(device)[..., None], lead(e["dk"]), lead(e["mag_dk"])),
                ("dv", "bias", v.grad, lead(e["dv"]), lead(e["mag_dv"])),
                ("dbias", "bias", bias.grad, e["d_bias"], e["mag_d_bias"])]
    return out, bias, geom


def run_packed(dtype, D, H, Hk, lens_q, lens_k, scale, l2norm_qk, device, causal=False, window=(-1, -1), max_seqlen=None, seed=0, grads=True):
    """flash_cosine_sim_attention_varlen on one probe per sequence, packed; the expectation of every distinct (N_s, M_s) computed once"""
    F = _F()
    qs, ks, vs, dos, rs, ms, memo, refs = [], [], [], [], [], [], {}, {n: [] for n in ("o", "dq", "dk", "dv", "mag_dq", "mag_dk")}
    for s, (n, mm) in enumerate(zip(lens_q, lens_k)):
        q, k, v, do, r, m = probe_inputs(dtype, 1, H, Hk, n, mm, D, l2norm_qk, seed + 2 * s)
        for lst, t in ((qs, q), (ks, k), (vs, v), (dos, do), (rs, r), (ms, m)):
            lst.append(t[0].transpose(0, 1))                              # [len, heads, ...]
        if not memo:
            spans = sorted(set(zip(lens_q, lens_k)))
            memo = {span: expected(vis, D, dtype, scale, l2norm_qk, grads=grads) for span, vis in zip(spans, vis_spans(*zip(*spans), causal, window))}
        for key in refs:
            if grads or key == "o":
                refs[key].append(memo[n, mm][key])
    cat = lambda lst: torch.cat(lst, 0).contiguous().to(device)
    q, k, v, do, r, m = (cat(x) for x in (qs, ks, vs, dos, rs, ms))
    if grads:
        q, k, v = (t.requires_grad_() for t in (q, k, v))
    cu = lambda lens: torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    o = F.flash_cosine_sim_attention_varlen(q, k, v, cu(lens_q), cu(lens_k), max_seqlen_q=max_seqlen, max_seqlen_k=max_seqlen, scale=scale,
                                            causal=causal, l2norm_qk=l2norm_qk, window_size=tuple(window))
    ref = {key: np.concatenate(val, 0)[:, None, :] for key, val in refs.items() if val}      # [total, 1, D] against [total, heads, D]
    out = [("o", "packed", o.detach(), ref["o"], ref["o"])]
    if grads:
        o.backward(do)
        G = H // Hk
        out += [("dq", "packed", q.grad * r[..., None], ref["dq"], ref["mag_dq"]),
                ("dk", "packed", k.grad * m[..., None], G * ref["dk"], G * ref["mag_dk"]),
                ("dv", "packed", v.grad, G * ref["dv"], G * ref["dv"])]
    return out


def _cache(dtype, D, B, Hk, cap, page, lens, l2norm_qk, seed, fp8_scales=None, first=0):
    """caches of B sequences whose first lens[b] positions hold the probe's keys by position (first + cache position: a shared prefix of
    `first` positions comes before them).  The slots behind a sequence's length hold
    valid probe keys whose VALUE class is one off, so a key read beyond the length moves a count and an append that lands nowhere leaves
    a wrong class behind.  Returns (k_cache, v_cache, block_table or None); paged caches go through a shuffled table into a pool with
    spare blocks."""
    k, v, _ = probe_keys(dtype, (B, Hk), cap, D, l2norm_qk, seed, pos=torch.arange(cap) + first)
    wrong = probe_keys(dtype, (B, Hk), cap, D, l2norm_qk, seed, pos=torch.arange(cap) + first + 1)[1]
    for b, n in enumerate(lens):
        v[b, :, n:] = wrong[b, :, n:]
    if fp8_scales is not None:
        k, v = ((t.double() / s).to(torch.float8_e4m3fn) for t, s in zip((k, v), fp8_scales))
    if not page:
        return k, v, None
    nb = cap // page
    perm = torch.randperm(B * nb + 3, generator=torch.Generator().manual_seed(seed))[:B * nb].to(torch.int32).view(B, nb)
    pools = []
    for t in (k, v):
        blocks = t.view(torch.uint8 if fp8_scales is not None else t.dtype).view(B, Hk, nb, page, D).permute(0, 2, 1, 3, 4).reshape(B * nb, Hk, page, D)
        pool = torch.zeros(B * nb + 3, Hk, page, D, dtype=blocks.dtype)
        pool[perm.view(-1).long()] = blocks
        pools.append(pool.view(t.dtype))
    return pools[0], pools[1], perm


def run_decode(dtype, D, H, Hk, N, cap, page, lens, n_new, counts, causal, fp8, scale, l2norm_qk, device, window=(-1, -1), append=True, seed=0,
               operand_dtype=None):
    """flash_cosine_sim_attention_with_kvcache (counts None: N rows per sequence, n_new appended keys) or ..._varlen_with_kvcache (counts:
    the ragged step; append: every query brings its key) with return_lse=True: o and lse of every sequence.  operand_dtype: the type the
    logit's operands are rounded to (default: q's)"""
    F = _F()
    B = len(lens)
    ragged = counts is not None
    rows = list(counts) if ragged else [N] * B
    news = ([n if append else 0 for n in rows] if ragged else [n_new] * B)
    scales = (0.5, 2.0) if fp8 else None
    kc, vc, table = _cache(dtype, D, B, Hk, cap, page, lens, l2norm_qk, seed + 7, scales)
    qs, kns, vns, refs_o, refs_l = [], [], [], [], []
    views = vis_ragged(rows, lens, append, causal, window) if ragged else [vis_cache(N, c, n_new, causal, window, cap) for c in lens]
    for b in range(B):
        q, _, _ = probe_queries(dtype, (H,), rows[b], D, l2norm_qk, seed + 3 * b)
        kn, vn, _ = probe_keys(dtype, (Hk,), news[b], D, l2norm_qk, seed + 3 * b + 1, pos=torch.arange(news[b]) + lens[b])
        qs.append(q), kns.append(kn), vns.append(vn)
        e = expected(views[b], D, operand_dtype or dtype, scale, l2norm_qk, grads=False)
        refs_o.append(e["o"]), refs_l.append(e["lse"])
    kw = dict(cache_seqlens=torch.tensor(lens, dtype=torch.int32), block_table=table, scale=scale, causal=causal, l2norm_qk=l2norm_qk,
              return_lse=True, window_size=tuple(window))
    if fp8:
        kw.update(k_scale=scales[0], v_scale=scales[1])
    kc, vc = kc.to(device), vc.to(device)
    with torch.no_grad():
        if ragged:
            q = torch.cat([t.transpose(0, 1) for t in qs], 0).contiguous().to(device)                       # [total_q, H, D]
            kn, vn = (torch.cat([t.transpose(0, 1) for t in x], 0).contiguous().to(device) if append else None for x in (kns, vns))
            cu = torch.tensor(np.concatenate([[0], np.cumsum(rows)]), dtype=torch.int32)
            o, lse = F.flash_cosine_sim_attention_varlen_with_kvcache(q, kc, vc, cu, kn, vn, **kw)
            ref_o, ref_l = np.concatenate(refs_o, 0)[:, None, :], np.concatenate(refs_l, 0)[:, None]
        else:
            q = torch.stack(qs).to(device)                                                                     # [B, H, N, D]
            kn, vn = (torch.stack(x).to(device) if n_new else None for x in (kns, vns))
            o, lse = F.flash_cosine_sim_attention_with_kvcache(q, kc, vc, kn, vn, **kw)
            ref_o, ref_l = np.stack(refs_o)[:, None], np.stack(refs_l)[:, None]
    return [("o", "decode", o, ref_o, ref_o), ("lse", "decode", lse, ref_l, None)]


def run_prefix(dtype, D, H, Hk, N, counts, cached, append, P, paged, causal, device, scale=8.0, seed=0):
    """flash_cosine_sim_attention_with_shared_prefix: a prefix of P positions (contiguous, or paged in a pool through prefix_block_table)
    in front of every sequence's own cache (capacity 64, contiguous), whose keys carry the classes of positions P, P + 1, ...; o and lse"""
    F = _F()
    B, cap, page = len(cached), 64, 16
    ragged = counts is not None
    rows = list(counts) if ragged else [N] * B
    news = [n if append else 0 for n in rows]
    kc, vc, _ = _cache(dtype, D, B, Hk, cap, 0, cached, True, seed + 5, first=P)
    pk, pv, ptable = _cache(dtype, D, 1, Hk, 2 * page, page if paged else 0, [P], True, seed + 9)
    qs, kns, vns, refs_o, refs_l = [], [], [], [], []
    for b in range(B):
        q, _, _ = probe_queries(dtype, (H,), rows[b], D, True, seed + 3 * b)
        kn, vn, _ = probe_keys(dtype, (Hk,), news[b], D, True, seed + 3 * b + 1, pos=torch.arange(news[b]) + P + cached[b])
        qs.append(q), kns.append(kn), vns.append(vn)
        vis = vis_shared_prefix(P, vis_cache(rows[b], cached[b], news[b], causal))
        e = expected(vis, D, dtype, scale, True, grads=False)              # (key positions 0 .. P + L - 1: the prefix, then the own cache)
        refs_o.append(e["o"]), refs_l.append(e["lse"])
    kw = dict(prefix_len=P, prefix_block_table=ptable, cache_seqlens=torch.tensor(cached, dtype=torch.int32), scale=scale, causal=causal,
              return_lse=True)
    kc, vc, pk, pv = (t.to(device) for t in (kc, vc, pk, pv))
    with torch.no_grad():
        if ragged:
            q = torch.cat([t.transpose(0, 1) for t in qs], 0).contiguous().to(device)
            kn, vn = (torch.cat([t.transpose(0, 1) for t in x], 0).contiguous().to(device) if append else None for x in (kns, vns))
            cu = torch.tensor(np.concatenate([[0], np.cumsum(rows)]), dtype=torch.int32)
            o, lse = F.flash_cosine_sim_attention_with_shared_prefix(q, pk, pv, kc, vc, cu_seqlens_q=cu, k_new=kn, v_new=vn, **kw)
            ref_o, ref_l = np.concatenate(refs_o, 0)[:, None, :], np.concatenate(refs_l, 0)[:, None]
        else:
            q = torch.stack(qs).to(device)
            kn, vn = (torch.stack(x).to(device) if append else None for x in (kns, vns))
            o, lse = F.flash_cosine_sim_attention_with_shared_prefix(q, pk, pv, kc, vc, k_new=kn, v_new=vn, **kw)
            ref_o, ref_l = np.stack(refs_o)[:, None], np.stack(refs_l)[:, None]
    return [("o", "prefix", o, ref_o, ref_o), ("lse", "prefix", lse, ref_l, None)]


def packed_cases():
    """the packed tables as the probe runs them: window_cases.PACKED_CASES and varlen_form_cases.CASES in one shape --
    id, dtype, D, query lengths, key lengths, H, Hk, max_seqlen, kwargs, window"""
    import varlen_form_cases as VF
    import window_cases as W
    out = []
    for name, dtype, D, H, Hk, left, right, kw, pad, mx in W.PACKED_CASES:
        lq, lk = list(VF.CORE_Q), list(VF.CORE_K)
        if pad is not None:
            lq += [(7 * j) % 23 for j in range(pad - len(VF.CORE_Q))]
            lk += [(5 * j + 3) % 19 for j in range(pad - len(VF.CORE_K))]
        out.append((name, dtype, D, lq, lk, H, Hk, mx, kw, (left, right)))
    for name, dtype, D, lq, lk, H, Hk, mx, kw in VF.CASES:
        out.append(("forms_" + name, dtype, D, lq, lk, H, Hk, mx, kw, (-1, -1)))
    return out


def decode_cases():
    """window_cases.DECODE_CASES and DECODE_PLAIN_CASES in one shape --
    id, dtype, D, H, Hk, N, capacity, page, lens, appended, counts, causal, fp8, kwargs, window"""
    import window_cases as W
    out = [(*c, (-1, -1)) for c in DECODE_PLAIN_CASES]
    for name, dtype, D, B, H, Hk, N, cap, page, lens, n_new, left, right, kw in W.DECODE_CASES:
        out.append(("window_" + name, dtype, D, H, Hk, N, cap, page, lens, n_new, None, kw.get("causal", False), False, kw, (left, right)))
    return out
