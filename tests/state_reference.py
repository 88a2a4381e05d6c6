"""float64 reference of the training-side attention states (flash_cosine_sim_attention_with_lse, merge_attention_states_with_grad):
torch autograd on the CPU over the plain composite -- grouped l2norm, logits, visibility, log-sum-exp, softmax, P V -- of
loss = <o, do> + <lse, dlse>.  operand_dtype ("bf16" | "f16"): the S product is fed the operands every 16-bit implementation feeds it
(oracle.rounded_operands: k^ rounded to the type, q^ rounded after c1 = scale * log2(e) is folded in), rounded straight-through, so the
gradient is the exact one of that forward with the rounding's own derivative taken as 1 -- "operand-faithful", as in the parity tests.
Rows without a visible key give o = 0 and lse = -inf and take no gradient; their dlse is ignored."""
import math

import torch

LOG2E = 1.0 / math.log(2.0)
F64 = torch.float64


def _round(x, operand_dtype):
    if operand_dtype == "bf16":
        return x.float().to(torch.bfloat16).to(F64)
    if operand_dtype == "f16":
        return x.to(torch.float16).to(F64)
    return x


def _l2norm(x, groups):
    g = x.unflatten(-1, (groups, x.shape[-1] // groups))
    return (g / torch.linalg.vector_norm(g, dim=-1, keepdim=True).clamp_min(1e-12)).flatten(-2)


def visible(N, M, causal=False, window=(-1, -1)):
    """[N, M] bool: query i of N sees key j of M iff i + (M - N) - left <= j <= i + (M - N) + right (-1: unbounded; causal: right = 0)"""
    left, right = window
    right = 0 if causal else right
    i = torch.arange(N)[:, None] + (M - N)
    j = torch.arange(M)[None, :]
    vis = torch.ones(N, M, dtype=torch.bool)
    if right >= 0:
        vis &= j <= i + right
    if left >= 0:
        vis &= j >= i - left
    return vis


def composite(q, k, v, scale=8.0, groups=1, causal=False, l2norm_qk=True, window=(-1, -1), operand_dtype=None):
    """(o, lse) in float64 from float64 q [B, H, N, D], k / v [B, Hk, M, D]; differentiable."""
    H, Hk = q.shape[1], k.shape[1]
    qh, kh = (_l2norm(q, groups), _l2norm(k, groups)) if l2norm_qk else (q, k)
    if l2norm_qk and operand_dtype in ("bf16", "f16"):
        c1 = abs(float(scale)) * LOG2E or 1.0
        qh = qh + (_round(qh.detach() * c1, operand_dtype) / c1 - qh.detach())
        kh = kh + (_round(kh.detach(), operand_dtype) - kh.detach())
    kh, vv = kh.repeat_interleave(H // Hk, dim=1), v.repeat_interleave(H // Hk, dim=1)
    s = torch.einsum("bhid,bhjd->bhij", qh, kh) * scale
    vis = visible(q.shape[2], k.shape[2], causal, window)
    live = vis.any(-1)                                                       # [N]
    neg = torch.full_like(s, float("-inf"))
    top = torch.where(vis, s, neg).amax(-1, keepdim=True).detach() if k.shape[2] else s.new_zeros(*s.shape[:-1], 1)
    top = torch.where(live[:, None], top, torch.zeros_like(top))
    e = torch.where(vis, torch.exp(torch.where(vis, s, torch.zeros_like(s)) - top), torch.zeros_like(s))
    l = torch.where(live, e.sum(-1), torch.ones_like(top[..., 0]))
    o = torch.einsum("bhij,bhjd->bhid", e / l[..., None], vv)
    lse = torch.where(live, top[..., 0] + torch.log(l), torch.full_like(l, float("-inf")))
    return o, lse


def reference(q, k, v, do, dlse, **kw):
    """(o, lse, dq, dk, dv) as float64 tensors: the composite and the gradients of <o, do> + <lse, dlse> (dlse None: 0) at the float64
    values of q, k, v (any dtype; dense 4-D)."""
    q, k, v = (t.detach().cpu().to(F64).requires_grad_() for t in (q, k, v))
    o, lse = composite(q, k, v, **kw)
    loss = (o * do.detach().cpu().to(F64)).sum()
    if dlse is not None:
        finite = torch.isfinite(lse)
        loss = loss + (torch.where(finite, lse, torch.zeros_like(lse)) * torch.where(finite, dlse.detach().cpu().to(F64), torch.zeros_like(lse))).sum()
    dq, dk, dv = torch.autograd.grad(loss, (q, k, v), allow_unused=True)
    zero = lambda g, t: torch.zeros_like(t) if g is None else g
    return o.detach(), lse.detach(), zero(dq, q), zero(dk, k), zero(dv, v)


def reference_packed(q, k, v, do, dlse, cu_q, cu_k, **kw):
    """`reference` on packed tensors (q [total_q, H, D], lse / dlse [total_q, H]), every sequence as a batch-1 problem."""
    o, lse = torch.zeros(q.shape, dtype=F64), torch.full(q.shape[:-1], float("-inf"), dtype=F64)
    dq, dk, dv = torch.zeros(q.shape, dtype=F64), torch.zeros(k.shape, dtype=F64), torch.zeros(v.shape, dtype=F64)
    for s in range(len(cu_q) - 1):
        a, b, c, d = cu_q[s], cu_q[s + 1], cu_k[s], cu_k[s + 1]
        if a == b:
            continue
        rows = lambda t, lo, hi: t[lo:hi].transpose(0, 1).unsqueeze(0)
        r = reference(rows(q, a, b), rows(k, c, d), rows(v, c, d), rows(do, a, b), None if dlse is None else dlse[a:b].transpose(0, 1).unsqueeze(0), **kw)
        o[a:b], lse[a:b] = r[0][0].transpose(0, 1), r[1][0].transpose(0, 1)
        dq[a:b], dk[c:d], dv[c:d] = r[2][0].transpose(0, 1), r[3][0].transpose(0, 1), r[4][0].transpose(0, 1)
    return o, lse, dq, dk, dv


def merge_composite(os, lses):
    """lse_reference.merge_reference's formula in differentiable float64 torch: (o, lse) of the merged state.  A state with lse = -inf is
    dropped before any arithmetic touches its o."""
    lse = torch.stack(list(lses))
    top = lse.amax(0).detach()
    live = torch.isfinite(top)
    safe = torch.where(live, top, torch.zeros_like(top))
    alive = torch.isfinite(lse)
    w = torch.where(alive, torch.exp(torch.where(alive, lse, torch.zeros_like(lse)) - safe), torch.zeros_like(lse))
    total = torch.where(live, w.sum(0), torch.ones_like(top))
    acc = sum(w[s][..., None] * torch.where(alive[s][..., None], o, torch.zeros_like(o)) for s, o in enumerate(os))
    return acc / total[..., None], torch.where(live, safe + torch.log(total), torch.full_like(top, float("-inf")))


def merge_reference_grads(os, lses, do, dlse):
    """(o, lse, [d o_s], [d lse_s]) in float64 for loss = <o, do> + <lse, dlse> (dlse None: 0)."""
    os = [t.detach().cpu().to(F64).requires_grad_() for t in os]
    lses = [t.detach().cpu().to(F64).requires_grad_() for t in lses]
    o, lse = merge_composite(os, lses)
    loss = (o * do.detach().cpu().to(F64)).sum()
    if dlse is not None:
        finite = torch.isfinite(lse)
        loss = loss + (torch.where(finite, lse, torch.zeros_like(lse)) * dlse.detach().cpu().to(F64)).sum()
    g = torch.autograd.grad(loss, os + lses, allow_unused=True)
    g = [torch.zeros_like(t) if x is None else x for x, t in zip(g, os + lses)]
    return o.detach(), lse.detach(), g[:len(os)], g[len(os):]
