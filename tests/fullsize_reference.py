"""References that are fast enough for full-size problems, for the dense, windowed, packed and decode calls alike.

Two kinds, both plain torch float64 on whatever device the inputs live on (test_fullsize_reference_cpu.py pins both to the numpy oracle on
the CPU; test_gpu_fullsize*.py and test_gpu_address_range.py run them on the GPU, where an N = 16384 slice takes milliseconds):

  * `attention_slice`: forward and (dq, dk, dv) of ONE slice -- a K/V head with its G query heads -- by the oracle's formulas
    (oracle.attention_forward_stats / attention_backward), in row blocks restricted to the band, so the logits of a block are at most
    row_block x (row_block + left + right) float64 values whatever N and M are.
  * the exact probes (`probe_v`, `probe_expected_o`, `probe_expected_dv`, `probe_compare`): structured inputs whose result is known in closed
    form for the WHOLE tensor, so every (batch / sequence, head, row) is judged, not a few slices.

`ref_slice` is the float32 / float64 slice reference of test_gpu_fullsize.py, moved here unchanged; `grads_operand_faithful` keeps its
signature and is now `attention_slice` with the 16-bit operands (the oracle's P~ / max(l, eps) instead of softmax, so a fully masked row
gives 0 instead of NaN; float16 operands in one rounding).

The rules below are the ones the suite already judges these operators by; the numbers are literals inside functions of the files named,
so they are restated here once, and test_fullsize_reference_cpu.py::test_restated_rules_still_stand_in_their_sources fails when a source
no longer carries them.
"""
import torch

LOG2E = 1.4426950408889634
REL_FLOOR = 1e-3                     # test_gpu_varlen.py::_rel: rel-L2 against max(||ref||, 1e-3 * sqrt(size))
GRAD_FLOOR = {"f32": 5e-2, "f16": 1e-3, "bf16": 1e-3}      # test_gpu_window.py::compare_slice / test_gpu_fuzz.py: the same floor for gradients
F32_ZERO_GRAD_ABS = 6e-6             # ... and float32's absolute allowance (x max(1, scale / 8) x sqrt(size)) where the exact gradient is 0
SHORT_SEQUENCE_FACTOR = 4.0          # test_gpu_varlen.py::_check / test_gpu_window.py seq_factor: a sequence under 100 rows on its own
SHORT_SEQUENCE_ROWS = 100
TANGENT_BAR = {"bf16": 6e-2, "f16": 1.5e-2, "f32": 1.5e-2}      # test_gpu_fullsize.py: the tangent-space identity
RESTATED_FROM = {
    "test_gpu_varlen.py": ("1e-3 * np.sqrt(max(b.size, 1))", "err <= 4 * (rel if nm == \"o\" else bar)"),
    "test_gpu_window.py": ("(5e-2 if dtype == \"f32\" else 1e-3) * np.sqrt(rr.size)", "err <= 6e-6 * max(1.0, scale / 8.0) * np.sqrt(rr.size)",
                           "seq_factor=4.0 if lq[s] < 100 else 1.0", "MODEL_SLACK = 2.0"),
    "test_gpu_fullsize.py": ("(6e-2 if bf else 1.5e-2)",),
}
DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def ref_slice(q, k, v, mask, causal, scale, groups, ref_dtype=torch.float32, operand_dtype=None):
    """PyTorch evaluation of softmax(scale * qn kn^T) v for [n, d] x [m, d] slices in `ref_dtype` (float32 or float64).
    operand_dtype: round the normalised operands to that dtype first -- c1 * q^ (c1 = scale * log2 e, as the kernels fold it) and
    k^ -- i.e. the "operand-faithful" reference: what exact arithmetic gives on the 16-bit operands every implementation of this op
    (the reference's too, py:57-65) feeds its S product.  It separates the error inherent to 16-bit operands, which grows with
    scale * groups, from everything else, so that check needs no range-dependent tolerance.  Differentiable (torch autograd)."""
    q, k, v = q.to(ref_dtype), k.to(ref_dtype), v.to(ref_dtype)
    d = q.shape[-1]

    def nrm(t):
        tg = t.reshape(t.shape[0], groups, d // groups)
        return torch.nn.functional.normalize(tg, dim=-1).reshape(t.shape)

    qn, kn = nrm(q), nrm(k)
    if operand_dtype is not None:
        c1 = scale * LOG2E
        qn = (qn * c1).to(operand_dtype).to(ref_dtype) / c1
        kn = kn.to(operand_dtype).to(ref_dtype)
    s = (qn @ kn.t()) * scale
    n, m = s.shape
    if causal:
        s = s.masked_fill(torch.ones(n, m, dtype=torch.bool, device=s.device).triu(m - n + 1), float("-inf"))
    if mask is not None:
        s = s.masked_fill(~mask[None, :], float("-inf"))
    return torch.softmax(s, dim=-1) @ v


def round_to(x, dtype):
    """float64 x rounded to a 16-bit dtype and back, as oracle.round_to does it on every device: bfloat16 through float32 (the oracle's bit
    trick works on float32), float16 in ONE rounding (numpy's float64 -> float16; torch's CPU conversion goes through float32, which
    rounds 6e-5 of random values to the other neighbour)."""
    if dtype == torch.bfloat16:
        return x.float().to(torch.bfloat16).double()
    assert dtype == torch.float16, dtype
    h = x.float().to(torch.float16).double()
    binade = torch.exp2(torch.floor(torch.log2(h.abs().clamp_min(2.0 ** -14))))
    ulp = binade / 1024
    # (below a power of two above the subnormal range the next value is half a step away: the finer binade)
    finer = torch.where((h.abs() == binade) & (binade > 2.0 ** -14), h - torch.sign(h) * ulp / 2, h)
    for c in (h - ulp, h + ulp, finer):
        h = torch.where((x - c).abs() < (x - h).abs(), c, h)
    return h


def window_sides(window, causal):
    """(left, right) with causal's cap of the right side at 0; -1: unbounded"""
    left, right = window
    return left, (0 if causal else right)


def visible_range(N, M, window, causal, device="cpu"):
    """(lo, hi, n): row i of N sees the keys lo[i] ... hi[i] of M (bottom-right alignment), n[i] = max(0, hi - lo + 1) of them; int64 [N]"""
    left, right = window_sides(window, causal)
    t = torch.arange(N, device=device, dtype=torch.int64) + (M - N)
    lo = torch.clamp(t - left, min=0) if left >= 0 else torch.zeros_like(t)
    hi = torch.clamp(t + right, max=M - 1) if right >= 0 else torch.full_like(t, M - 1)
    return lo, hi, torch.clamp(hi - lo + 1, min=0)


def seeing_rows(N, M, window, causal, device="cpu"):
    """(a, b): key j of M is seen by the rows a[j] ... b[j] of N (an interval; empty where b < a); int64 [M]"""
    left, right = window_sides(window, causal)
    j = torch.arange(M, device=device, dtype=torch.int64)
    off = M - N
    a = torch.clamp(j - right - off, min=0) if right >= 0 else torch.zeros_like(j)
    b = torch.clamp(j + left - off, max=N - 1) if left >= 0 else torch.full_like(j, N - 1)
    return a, b


def zero_gradient_rows(N, M, window, causal, device="cpu"):
    """(q rows, k rows) whose dq / dk are 0 in exact math by the structure of the problem alone: a query that sees at most one key has
    P = 1 there, so dS = 0; a key seen only by such queries (or by none) collects no dS.  bool [N], bool [M]"""
    _, _, n = visible_range(N, M, window, causal, device=device)
    live = torch.zeros(N + 1, dtype=torch.int64, device=device)
    live[1:] = torch.cumsum((n > 1).to(torch.int64), dim=0)
    a, b = seeing_rows(N, M, window, causal, device=device)
    b = torch.maximum(b, a - 1)
    return n <= 1, (live[torch.clamp(b + 1, min=0, max=N)] - live[torch.clamp(a, max=N)]) == 0


def attention_slice(q, k, v, do=None, *, scale=8.0, groups=1, causal=False, window=(-1, -1), l2norm_qk=True, eps=1e-10, operand_dtype=None,
                    mask=None, o_saved=None, row_block=512):
    """One K/V head with its G query heads in float64: q, do, o_saved [G, N, D], k, v [M, D], mask [M] bool or None.
    Returns o [G, N, D], or (o, dq [G, N, D], dk [M, D], dv [M, D]) when `do` is given; dk / dv are summed over the group.

    The math is the oracle's, term for term: P~ = visible ? exp(S - scale) : 0, l = rowsum P~, P = P~ / max(l, eps) (eps: 1e-10 in the
    static shift regime, 1e-300 where cases.dynamic_shift_regime says the rows are normalised exactly), o = P v, delta = rowsum(dO * o)
    (o_saved: the stored output instead, as a backward pass reads it), dv = P^T dO, dS = P * (dO v^T - delta), dq^ = scale dS k^,
    dk^ = scale dS^T q^, then the l2norm backward.  operand_dtype (a torch 16-bit dtype): c1 * q^ and k^ are rounded to it before the S
    product and stand in for x / |x| in the l2norm backward (oracle.rounded_operands: the "operand-faithful" twin).
    window = (left, right), -1 unbounded, bottom-right aligned for N != M; causal caps right at 0.  Rows without a visible key give 0."""
    q, k, v = q.double(), k.double(), v.double()
    G, N, D = q.shape
    M = k.shape[0]
    dev = q.device
    scale = float(scale)

    def nrm(t):
        tg = t.reshape(*t.shape[:-1], groups, D // groups)
        inv = 1.0 / tg.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        return (tg * inv).reshape(t.shape), inv

    qh, rq = nrm(q) if l2norm_qk else (q, None)
    kh, rk = nrm(k) if l2norm_qk else (k, None)
    if operand_dtype is not None and operand_dtype != torch.float32:
        c1 = abs(scale) * LOG2E
        c1 = c1 if c1 > 0 else 1.0
        qh = round_to(qh * c1, operand_dtype) / c1
        kh = round_to(kh, operand_dtype)
    left, right = window_sides(window, causal)
    off = M - N
    o = torch.zeros_like(q)
    grads = do is not None
    if grads:
        do = do.double()
        dqh, dkh, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
        o_used = None if o_saved is None else o_saved.double()
    for g in range(G):
        for r0 in range(0, N, row_block):
            r1 = min(N, r0 + row_block)
            c0 = 0 if left < 0 else max(0, r0 + off - left)
            c1_ = M if right < 0 else min(M, r1 + off + right)
            if c1_ <= c0:
                continue
            i = torch.arange(r0, r1, device=dev)[:, None] + off
            j = torch.arange(c0, c1_, device=dev)[None, :]
            ok = torch.ones((r1 - r0, c1_ - c0), dtype=torch.bool, device=dev)
            if left >= 0:
                ok &= j >= i - left
            if right >= 0:
                ok &= j <= i + right
            if mask is not None:
                ok &= mask[None, c0:c1_]
            kb, vb = kh[c0:c1_], v[c0:c1_]
            s = (qh[g, r0:r1] @ kb.t()) * scale
            p = torch.where(ok, torch.exp(s - scale), torch.zeros_like(s))
            p = p / p.sum(-1, keepdim=True).clamp_min(eps)
            ob = p @ vb
            o[g, r0:r1] = ob
            if grads:
                dob = do[g, r0:r1]
                delta = (dob * (ob if o_used is None else o_used[g, r0:r1])).sum(-1, keepdim=True)
                dv[c0:c1_] += p.t() @ dob
                ds = p * (dob @ vb.t() - delta)
                dqh[g, r0:r1] = scale * (ds @ kb)
                dkh[c0:c1_] += scale * (ds.t() @ qh[g, r0:r1])
    if not grads:
        return o

    def nrm_bwd(gr, xh, inv):
        gg, xg = gr.reshape(*gr.shape[:-1], groups, -1), xh.reshape(*gr.shape[:-1], groups, -1)
        return (inv * (gg - xg * (gg * xg).sum(-1, keepdim=True))).reshape(gr.shape)

    if l2norm_qk:
        return o, nrm_bwd(dqh, qh, rq), nrm_bwd(dkh, kh, rk), dv
    return o, dqh, dkh, dv


def grads_operand_faithful(q, k, v, do, mask, causal, scale, groups, dtype):
    """Gradients of one (batch, head) slice ([n, d] x [m, d]) by the kernel's own formulas in float64 on the 16-bit
    OPERANDS: c1 * q^ and k^ rounded to `dtype` feed S, dQ^ = scale dS K^, dK^ = scale dS^T Q^ and the projection of the l2norm backward
    (what oracle.attention_backward(operand_dtype=...) computes, here in torch on the GPU so that full-size slices take milliseconds).
    Rows are normalised exactly (no clamp).  Returns (dq, dk, dv) w.r.t. the raw slices."""
    _, dq, dk, dv = attention_slice(q[None], k, v, do[None], scale=scale, groups=groups, causal=causal, mask=mask, eps=1e-300, operand_dtype=dtype)
    return dq[0], dk, dv


# ---- exact probes -----------------------------------------------------------------------------------------------------------------------
#
# Uniform attention: every q row and every valid k row is the same vector, so all logits of a row are equal and P is exactly uniform over
# the row's n_i visible keys.  v is 0 except for "sentinels": feature f of a (sequence, K/V head) unit is a power of two at ONE key s_f.
# Then o[i, f] is exactly 0 iff s_f is not visible to row i, and VALUE / n_i otherwise -- each sentinel is an exact off-by-one test of both
# band edges, of the sequence's first and last key, and of the address of V row s_f.  With uniform P, dv[j] = sum_{i sees j} dO[i] / n_i:
# the rows that see j are an interval, so this is a difference of one prefix sum over the rows.
#
# What the probes do NOT see: all valid K rows are equal, so a mis-addressed VALID K row goes unnoticed (the random-data slices and the
# bit-for-bit address tests are for that), and in the 16-bit types a wrong key COUNT in a wide window is below one output ulp unless a
# sentinel sits on the affected position (the f32 probes resolve every count: 1 / n_i differs from 1 / (n_i + 1) by 2^-15 at n = 32768).

VALUE = 16.0      # 16 / 32768 keys = 2^-11: a normal number in float16 (smallest normal 2^-14), bfloat16 and float32
EDGE_RESIDUES = (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255)      # key positions mod 256 next to a 64- / 128- / 256-key tile edge


def unit_vector(D, dtype):
    """the one q / k row of the probes: unit norm before rounding (so l2norm_qk = False cases take it as it is), mixed signs and magnitudes"""
    d = torch.arange(D, dtype=torch.float64)
    u = (1.0 + (d % 3)) * torch.where(d % 2 == 0, 1.0, -1.0)
    return (u / u.norm()).to(dtype)


def sentinel_positions(unit, L, D):
    """key position of the sentinel of every feature of (sequence, K/V head) unit number `unit` (any integer), for a sequence of L keys:
    int64 [D], deterministic.  Features 0 / 1 take the first / last key; the others go through every residue of EDGE_RESIDUES on a
    256-key tile that moves with (unit, feature), so that over the heads of a case the sentinels spread over the whole length."""
    f = torch.arange(D, dtype=torch.int64)
    tiles = max(1, (L + 255) // 256)
    tile = (f * 7 + unit * 13 + (f // len(EDGE_RESIDUES)) * 5) % tiles
    pos = (tile * 256 + torch.tensor(EDGE_RESIDUES, dtype=torch.int64)[(f + unit) % len(EDGE_RESIDUES)]) % max(L, 1)
    pos[0] = 0
    if D > 1:
        pos[1] = max(L - 1, 0)
    return pos


def probe_v(units, L, D, dtype, device="cpu"):
    """v [len(units), L, D] of the sentinels of the given unit numbers, and their positions [len(units), D]"""
    pos = torch.stack([sentinel_positions(u, L, D) for u in units]).to(device)
    v = torch.zeros((len(units), L, D), dtype=dtype, device=device)
    if L > 0:
        v.scatter_(1, pos[:, None, :], torch.full((len(units), 1, D), VALUE, dtype=dtype, device=device))
    return v, pos


def probe_expected_o(N, M, window, causal, pos):
    """closed-form o [N, D] (float64) of a unit whose sentinels sit at pos [D]: VALUE / n_i where lo_i <= pos_f <= hi_i, else exactly 0"""
    lo, hi, n = visible_range(N, M, window, causal, device=pos.device)
    seen = (pos[None, :] >= lo[:, None]) & (pos[None, :] <= hi[:, None])
    return torch.where(seen, VALUE / n.clamp_min(1).double()[:, None], torch.zeros((), dtype=torch.float64, device=pos.device))


def probe_expected_dv(do, M, window, causal):
    """closed-form dv [M, D] (float64) of uniform attention: do [G, N, D] of the group's query heads.  Key j is seen by the rows
    a_j ... b_j with a_j = j - right - (M - N), b_j = j + left - (M - N), clipped to [0, N - 1]: dv[j] = C[b_j + 1] - C[a_j] with C the
    prefix sum of dO[i] / n_i over the rows (rows without a visible key see nothing and add nothing)."""
    G, N, D = do.shape
    dev = do.device
    _, _, n = visible_range(N, M, window, causal, device=dev)
    w = torch.where(n > 0, 1.0 / n.clamp_min(1).double(), torch.zeros((), dtype=torch.float64, device=dev))
    c = torch.zeros((N + 1, D), dtype=torch.float64, device=dev)
    c[1:] = torch.cumsum(do.double().sum(0) * w[:, None], dim=0)
    a, b = seeing_rows(N, M, window, causal, device=dev)
    b = torch.maximum(b, a - 1)                       # (an empty interval: a key no row sees)
    a = torch.clamp(a, max=N)
    return c[torch.clamp(b + 1, min=0, max=N)] - c[a]


def probe_compare(got, expected):
    """(the zero pattern is exact, worst relative error of the non-zero values) of an output against its closed form; no absolute term"""
    got, expected = got.double(), expected.double()
    zero = expected == 0
    pattern = bool(torch.equal(got == 0, zero))
    nz = ~zero
    rel = float(((got[nz] - expected[nz]).abs() / expected[nz].abs()).max().item()) if bool(nz.any()) else 0.0
    return pattern, rel


def sequence_of_cache(cache, b, L, table=None):
    """positions [0, L) of sequence b as the expectation side reads a cache: [Hk, L, D].  Contiguous caches are [B, Hk, capacity, D], paged
    ones [num_blocks, Hk, page, D] with table[b, i] naming the block of positions [i * page, (i + 1) * page)."""
    if table is None:
        return cache[b, :, :L]
    page = cache.shape[2]
    nb = (L + page - 1) // page
    if nb == 0:
        return cache[0, :, :0]
    blocks = table[b, :nb].to(device=cache.device, dtype=torch.int64)
    return cache[blocks].permute(1, 0, 2, 3).reshape(cache.shape[1], nb * page, cache.shape[3])[:, :L]


def probe_expected_sequence(vseq, N, window, causal, G):
    """closed-form o [Hk * G, N, D] (float64) of one sequence from its probe values vseq [Hk, L, D] AS THE EXPECTATION SIDE GATHERED THEM:
    the sentinel of feature f is where vseq[h, :, f] is largest, so a wrong table entry or sequence offset on this side moves it"""
    Hk, L, D = vseq.shape
    if L == 0 or N == 0:
        return torch.zeros((Hk * G, N, D), dtype=torch.float64, device=vseq.device)
    pos = vseq.float().argmax(dim=1)
    o = torch.stack([probe_expected_o(N, L, window, causal, pos[h]) for h in range(Hk)])
    return o.repeat_interleave(G, dim=0)
