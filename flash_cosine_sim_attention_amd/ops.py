"""Public operator API -- same names, keywords and defaults as the reference package
(flash_cosine_sim_attention/__init__.py:1, flash_cosine_sim_attention.py:308-334).

Differences from the reference, all inside the boundary:
  * the (grouped) l2norm of q and k is FUSED into the op (q in the forward kernel's prologue, k in
    a library row kernel, inverse norms saved; the l2norm backward in the dQ / dKV epilogues)
    instead of two eager F.normalize passes outside the autograd.Function
    (flash_cosine_sim_attention.py:320-321), so `FlashCosineSimAttention.backward` returns
    gradients w.r.t. the RAW q, k;
  * GPU tensors only ever run on the hand-written gfx950 kernels; there is no silent fallback
    (a missing libfcsa_hip.so raises ImportError).  CPU tensors take this package's own
    forward-only blockwise path (`cpu.py`), as they do in the reference (py:322-323).

Logit range: with l2norm_qk the logits lie in +-|scale|*groups.  Inside the library's static exponent window (f16: <= 11 and no attn_bias,
bf16 / f32: <= 75) the kernels use one constant shift like the reference (whose kernel overflows / zeroes rows at the far end of that
range); beyond it the forward shifts every row by its own max logit and normalises exactly, like the reference's PyTorch
plain_cosine_sim_attention.  There is no limit on scale (only float16 refuses |scale| * log2(e) > 60000).
"""
from __future__ import annotations

import types

import torch
from torch.autograd import Function

from . import _lib
from . import _torch_ops
from . import cpu as _cpu


# ---------------------------------------------------------------------------------------------
# l2norm helpers: public exports of the reference package (flash_cosine_sim_attention.py:38-65).
# Differentiable torch code; the fused operator does not call them.
# ---------------------------------------------------------------------------------------------

def _norm_floor(t: torch.Tensor) -> float:
    # the reference clamps the norm at F.normalize's 1e-12 on the GPU and, on the CPU, at 1e-3 for the 16-bit types (py:38-48)
    return 1e-12 if (t.is_cuda or t.dtype == torch.float32) else 1e-3


def l2norm(t):
    """t / max(||t||_2, eps) over the last dimension."""
    length = torch.linalg.vector_norm(t, dim=-1, keepdim=True)
    return t / length.clamp_min(_norm_floor(t))


def grouped_l2norm(t, groups=1):
    """l2norm of each of `groups` equal slices of the last dimension."""
    width = t.shape[-1]
    if groups < 1 or width % groups:
        raise ValueError(f"groups ({groups}) must divide the last dimension ({width})")
    return l2norm(t.unflatten(-1, (groups, width // groups))).flatten(-2)


def l2norm_tensors(*tensors, groups=1):
    """Grouped l2norm of every tensor, each cast to the dtype of the FIRST one (py:57-65)."""
    if not tensors:
        raise ValueError("l2norm_tensors needs at least one tensor")
    target = tensors[0].dtype
    return tuple(grouped_l2norm(t, groups).to(target) for t in tensors)


# ---------------------------------------------------------------------------------------------
# O(N*M)-memory attention in plain PyTorch ops: the reference's `plain_cosine_sim_attention`
# (py:75-126), kept as a public export.  Runs wherever its inputs live.  Not used by the fused op.
# ---------------------------------------------------------------------------------------------

def plain_cosine_sim_attention(q, k, v, mask=None, attn_bias=None, scale=8, groups=1, causal=False,
                               l2norm_qk=True, attn_bias_batch_dim=False):
    if causal and mask is not None:
        raise AssertionError("mask should not be supplied if causality is needed")
    squeeze_heads = q.dim() == 3                       # merged batch-heads queries
    if squeeze_heads:
        if k.dim() != 3 or v.dim() != 3:
            raise AssertionError("if batch and heads are merged for queries, keys and values must also similarly have only 3 dimensions")
        attn_bias_batch_dim, q = True, q.unsqueeze(1)
    q, k = l2norm_tensors(q, k, groups=groups) if l2norm_qk else (q, k)
    # single-headed K/V broadcast over the heads; grouped-query K/V (Hk dividing H) repeated over each group
    keys = _cpu.expand_kv_heads(k.unsqueeze(1) if k.dim() == 3 else k, q.shape[1])
    values = _cpu.expand_kv_heads(v.unsqueeze(1) if v.dim() == 3 else v, q.shape[1])
    logits = torch.matmul(q, keys.transpose(-1, -2)) * scale
    if attn_bias is not None:
        logits = logits + attn_bias.unsqueeze(1 if attn_bias_batch_dim else 0)
    lowest = -torch.finfo(logits.dtype).max
    n, m = logits.shape[-2:]
    if causal:                                         # key j is visible to query i iff j - (m - n) <= i
        future = torch.ones((n, m), dtype=torch.bool, device=logits.device).triu(m - n + 1)
        logits = logits.masked_fill(future, lowest)
    if mask is not None:
        logits = logits.masked_fill(~mask[:, None, None, :], lowest)
    out = torch.matmul(logits.softmax(dim=-1), values)
    return out.squeeze(1) if squeeze_heads else out


# ---------------------------------------------------------------------------------------------
# autograd.Function (flash_cosine_sim_attention.py:245-304) with the l2norm fused in
# ---------------------------------------------------------------------------------------------

class FlashCosineSimAttention(Function):
    """The reference's autograd.Function name (py:245), kept as a public export: a thin Python Function over the compiled
    dispatcher ops `torch.ops.fcsa.forward / backward`.  `flash_cosine_sim_attention` itself uses the same two ops through a
    C++ autograd node (`torch.ops.fcsa.attention`), which saves the ~60 us a Python Function costs per forward+backward."""

    @staticmethod
    def forward(ctx, q, k, v, mask, attn_bias, scale, groups, causal, l2norm_qk, attn_bias_batch_dim):
        if not q.is_cuda:
            raise RuntimeError("flash_cosine_sim_attention_amd: q, k, v must be GPU tensors (HIP kernels only, no CPU fallback)")
        fc = _torch_ops.load()
        should_backwards = any(ctx.needs_input_grad[i] for i in (0, 1, 2, 4))              # q, k, v, attn_bias (cu:1689)
        o, inv_l, qn, kn, rq, rk = fc.forward(q, k, v, mask, attn_bias, bool(attn_bias_batch_dim), float(scale), bool(causal),
                                              bool(l2norm_qk), int(groups), should_backwards)
        ctx.should_backwards = should_backwards
        if not should_backwards:
            return o
        # tensors go through save_for_backward (py:270): no reference cycle through ctx, in-place modification of a saved
        # input is detected, saved-tensor hooks (checkpointing, offload) apply; scalars stay plain attributes
        ctx.save_for_backward(o, inv_l, q, k, v, mask, attn_bias, qn, kn, rq, rk)
        ctx.scalars = (bool(attn_bias_batch_dim), float(scale), bool(causal), bool(l2norm_qk), int(groups))
        ctx.bias_grad = bool(attn_bias is not None and ctx.needs_input_grad[4])
        return o

    @staticmethod
    def backward(ctx, do):
        assert ctx.should_backwards
        o, inv_l, q, k, v, mask, attn_bias, qn, kn, rq, rk = ctx.saved_tensors
        dq, dk, dv, db = _torch_ops.load().backward(do, o, inv_l, q, k, v, mask, attn_bias, qn, kn, rq, rk, *ctx.scalars,
                                                    ctx.bias_grad)
        return dq, dk, dv, None, (db if ctx.bias_grad else None), None, None, None, None, None


flash_cosine_sim_attention_hip = FlashCosineSimAttention.apply


def flash_cosine_sim_attention(q, k, v, mask=None, attn_bias=None, scale=8, groups=1, causal=False,
                               l2norm_qk=True, attn_bias_batch_dim=False):
    """Fused cosine-similarity attention; signature of flash_cosine_sim_attention.py:308-319.

    GPU tensors: hand-written gfx950 kernels, forward and backward (gradients w.r.t. the raw q, k, v, attn_bias).
    k, v: [B, Hk, M, D] with Hk dividing H (Hk == H; grouped-query attention, query head h attending to K/V head h // (H // Hk);
    or 3-D single-headed K/V); dk, dv have the shape of k, v (sums over each group's query heads).
    CPU tensors: forward-only blockwise path (`cpu.attention_forward_cpu`), like the reference (py:322-323).
    Any finite scale runs (see the module docstring for the exponent-shift regimes)."""
    if q.device.type == "cpu":
        return _cpu.attention_forward_cpu(q, k, v, mask=mask, attn_bias=attn_bias, scale=scale, groups=groups, causal=causal,
                                          l2norm_qk=l2norm_qk, attn_bias_batch_dim=attn_bias_batch_dim)
    # the differentiable dispatcher op: autograd node, checks, allocation and launches all in C++ (csrc/fcsa_torch.cpp)
    return _torch_ops.load().attention(q, k, v, mask, attn_bias, bool(attn_bias_batch_dim), float(scale), bool(causal),
                                       bool(l2norm_qk), int(groups))


# ---------------------------------------------------------------------------------------------
# sliding-window (local) attention (flash-attn's window_size convention; no reference counterpart)
# ---------------------------------------------------------------------------------------------

def _window(window_size):
    """(left, right) as two ints >= -1 (any integer type; no bool, no float): the rule of `cpu.window_index`."""
    return _cpu.window_index(window_size)


def flash_cosine_sim_attention_local(q, k, v, window_size, scale=8, groups=1, causal=False, l2norm_qk=True):
    """Fused cosine-similarity attention under a sliding window: query i of N sees key j of M iff
    i + (M - N) - left <= j <= i + (M - N) + right, with window_size = (left, right), -1 for an unbounded side and the bottom-right
    alignment `causal` uses; causal=True caps right at 0.  Rows without a visible key give 0 (and zero gradients).  Otherwise
    `flash_cosine_sim_attention` without mask and attn_bias: 4-D q, k, v (k, v heads dividing q's), differentiable w.r.t. q, k, v.
    Only the tiles of the band are visited, so time and traffic go with N * (left + right), not N * M.  A window that hides no pair
    of the problem -- and (-1, 0), which is causal=True -- runs the un-windowed kernels, bit for bit.
    CPU tensors take the forward-only path of `cpu.py`."""
    left, right = _window(window_size)
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError("flash_cosine_sim_attention_local takes 4-D q, k, v ([batch, heads, length, dim_head])")
    if q.device.type == "cpu":
        return _cpu.attention_forward_cpu(q, k, v, scale=scale, groups=groups, causal=causal, l2norm_qk=l2norm_qk, window_size=(left, right))
    return _torch_ops.load().window_attention(q, k, v, float(scale), bool(causal), bool(l2norm_qk), int(groups), left, right)


# ---------------------------------------------------------------------------------------------
# packed variable-length sequences (the flash-attn cu_seqlens convention; no reference counterpart)
# ---------------------------------------------------------------------------------------------

def _check_host_cu(name, cu, total, max_len):
    """Full validation of a HOST table: cu[0] == 0, non-decreasing, cu[-1] == total, every span <= max_len (when given)."""
    c = cu.tolist()
    if c[0] != 0 or c[-1] != total:
        raise ValueError(f"{name} must start at 0 and end at the packed length {total}, got {c[0]} ... {c[-1]}")
    lens = [b - a for a, b in zip(c[:-1], c[1:])]
    if any(n < 0 for n in lens):
        raise ValueError(f"{name} must be non-decreasing")
    longest = max(lens, default=0)
    if max_len is not None and longest > max_len:
        raise ValueError(f"{name}: a sequence of {longest} rows is longer than max_seqlen = {max_len}")
    return longest


def _check_packed(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k):
    """The checks of a packed call (`flash_cosine_sim_attention_varlen`, `flash_cosine_sim_attention_with_lse`): shapes, dtypes, tables;
    host tables are validated fully.  Returns (max_seqlen_q, max_seqlen_k), filled in from host tables where they were None."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dim() != 3:
            raise ValueError(f"{name} must be a packed [total, heads, dim_head] tensor, got {tuple(t.shape)}")
    if k.shape != v.shape:
        raise ValueError(f"k and v must have the same shape, got {tuple(k.shape)} and {tuple(v.shape)}")
    if q.shape[2] != k.shape[2]:
        raise ValueError("query, key, value dimensions must be the same")
    if not (q.dtype == k.dtype == v.dtype) or q.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"q, k, v must share one of float32, float16, bfloat16, got {q.dtype}, {k.dtype}, {v.dtype}")
    if k.shape[1] < 1 or q.shape[1] % k.shape[1]:
        raise ValueError(f"k/v heads must divide q heads ({q.shape[1]}), got {k.shape[1]}")
    for name, cu in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if not isinstance(cu, torch.Tensor) or cu.dtype != torch.int32 or cu.dim() != 1 or cu.numel() < 1:
            raise TypeError(f"{name} must be a 1-D int32 tensor of sequences + 1 entries")
    if cu_seqlens_q.numel() != cu_seqlens_k.numel():
        raise ValueError("cu_seqlens_q and cu_seqlens_k must have the same length (sequences + 1)")
    for name, m in (("max_seqlen_q", max_seqlen_q), ("max_seqlen_k", max_seqlen_k)):
        if m is not None and (int(m) != m or m < 0):
            raise ValueError(f"{name} must be a non-negative integer, got {m}")
    if cu_seqlens_q.device.type == "cpu":
        longest = _check_host_cu("cu_seqlens_q", cu_seqlens_q, q.shape[0], max_seqlen_q)
        max_seqlen_q = longest if max_seqlen_q is None else max_seqlen_q
    if cu_seqlens_k.device.type == "cpu":
        longest = _check_host_cu("cu_seqlens_k", cu_seqlens_k, k.shape[0], max_seqlen_k)
        max_seqlen_k = longest if max_seqlen_k is None else max_seqlen_k
    if q.device.type == "cpu" and (cu_seqlens_q.device.type != "cpu" or cu_seqlens_k.device.type != "cpu"):
        raise ValueError("CPU tensors take host cu_seqlens tables")
    return max_seqlen_q, max_seqlen_k


def _packed_on_device(q, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k):
    """(cu_seqlens_q, cu_seqlens_k on q's device, max_seqlen_q, max_seqlen_k as ints): device tables are trusted; a max_seqlen left to us
    costs one device synchronisation per table."""
    if max_seqlen_q is None:
        max_seqlen_q = int((cu_seqlens_q[1:] - cu_seqlens_q[:-1]).max().item()) if cu_seqlens_q.numel() > 1 else 0
    if max_seqlen_k is None:
        max_seqlen_k = int((cu_seqlens_k[1:] - cu_seqlens_k[:-1]).max().item()) if cu_seqlens_k.numel() > 1 else 0
    return cu_seqlens_q.to(q.device, non_blocking=True), cu_seqlens_k.to(q.device, non_blocking=True), int(max_seqlen_q), int(max_seqlen_k)


def _dense_or_packed(name, q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k):
    """The opening of the functions that take 4-D q, k, v, or packed 3-D ones with both tables (`name`: the function, for its messages).
    Returns (packed, max_seqlen_q, max_seqlen_k), the latter two as `_check_packed` leaves them."""
    packed = cu_seqlens_q is not None or cu_seqlens_k is not None
    if packed:
        if cu_seqlens_q is None or cu_seqlens_k is None:
            raise ValueError("cu_seqlens_q and cu_seqlens_k must be given together")
        max_seqlen_q, max_seqlen_k = _check_packed(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k)
    else:
        if max_seqlen_q is not None or max_seqlen_k is not None:
            raise ValueError("max_seqlen_q / max_seqlen_k belong to packed calls (cu_seqlens_q, cu_seqlens_k)")
        if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
            raise ValueError(f"{name} takes 4-D q, k, v ([batch, heads, length, dim_head]), or packed 3-D ones "
                             "with cu_seqlens_q and cu_seqlens_k")
    return packed, max_seqlen_q, max_seqlen_k


def flash_cosine_sim_attention_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q=None, max_seqlen_k=None, scale=8, groups=1,
                                      causal=False, l2norm_qk=True, window_size=(-1, -1)):
    """Fused cosine-similarity attention over packed variable-length sequences.

    q [total_q, H, D] and k, v [total_k, Hk, D] (Hk dividing H) hold S sequences back to back; sequence s owns the query rows
    [cu_seqlens_q[s], cu_seqlens_q[s + 1]) and the key rows [cu_seqlens_k[s], cu_seqlens_k[s + 1]) (int32 tables of S + 1 entries).
    Each sequence's output rows are what `flash_cosine_sim_attention` returns for that sequence alone as a [1, H, N_s, D] problem
    (causal alignment per sequence, rows without a visible key give 0).  Returns o shaped like q; differentiable w.r.t. q, k, v.
    There is no mask or attn_bias.

    Tables on the host are validated fully (and copied to q's device); tables already on the device are trusted, as in flash-attn --
    a malformed device table gives wrong rows, never an access outside the tensors.  max_seqlen_q / max_seqlen_k must be at least
    the longest span: the launch grid is sized by them.  When None they are computed from the tables, which synchronises the device
    when the tables live there.  CPU tensors take the forward-only path of `cpu.py`, one dense CPU call per sequence.
    window_size = (left, right): a sliding window as in `flash_cosine_sim_attention_local`, every sequence with its own alignment."""
    window = _window(window_size)
    max_seqlen_q, max_seqlen_k = _check_packed(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k)
    if q.device.type == "cpu":
        return _cpu.attention_forward_varlen_cpu(q, k, v, cu_seqlens_q, cu_seqlens_k, scale=scale, groups=groups, causal=causal,
                                                 l2norm_qk=l2norm_qk, window_size=window)
    cu_q, cu_k, max_seqlen_q, max_seqlen_k = _packed_on_device(q, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k)
    if window != (-1, -1):
        return _torch_ops.load().varlen_window_attention(q, k, v, cu_q, cu_k, int(max_seqlen_q), int(max_seqlen_k), float(scale),
                                                         bool(causal), bool(l2norm_qk), int(groups), window[0], window[1])
    return _torch_ops.load().varlen_attention(q, k, v, cu_q, cu_k, int(max_seqlen_q), int(max_seqlen_k), float(scale), bool(causal),
                                              bool(l2norm_qk), int(groups))


# ---------------------------------------------------------------------------------------------
# a linear position bias (ALiBi) in training: dense, local and packed calls with per-head slopes, forward and backward
# ---------------------------------------------------------------------------------------------

def flash_cosine_sim_attention_alibi(q, k, v, alibi_slopes, scale=8, groups=1, causal=False, l2norm_qk=True, window_size=(-1, -1),
                                     cu_seqlens_q=None, cu_seqlens_k=None, max_seqlen_q=None, max_seqlen_k=None):
    """`flash_cosine_sim_attention` (4-D q, k, v), `flash_cosine_sim_attention_local` (with a window_size) or
    `flash_cosine_sim_attention_varlen` (packed 3-D q, k, v with cu_seqlens_q / cu_seqlens_k) with a linear position bias applied in
    registers: the training side of `flash_cosine_sim_attention_alibi_with_kvcache`, differentiable w.r.t. q, k, v.

    alibi_slopes: a float32 tensor [H] or [B, H] (B: the batch, or the number of sequences of a packed call), indexed by the QUERY head, so
    with grouped K/V every query head keeps its own slope.  With pos_i = i + M - N (the bottom-right alignment of causal and of the
    window, per sequence when packed) the logit of key j gains -alibi_slopes[b, h] * |pos_i - j|, in natural units after scale: the
    definition of the cached call, so a trained model is served unchanged.  Nothing of size [H, N, M] is read or written, and a window
    or packed sequences -- which refuse attn_bias -- combine with it.
    Slopes must be >= 0: the bias is a penalty.  Host slopes are checked (finite, non-negative) and moved to q's device without blocking;
    device slopes are trusted and never read on the host, so the call does not synchronise and can be captured in a graph (slopes
    changed in place are picked up on replay).  A negative device slope is numerically undefined, never an access out of bounds.
    There is no slope gradient (alibi_slopes.requires_grad is refused), no mask and no attn_bias.
    Numerics: the bias is <= 0, so the call runs the exponent regime of the same call without slopes (bfloat16 / float32, and float16 up
    to scale * groups = 11, keep the static shift); a weight that underflows is an exact 0.  Zero slopes equal the local / packed windowed
    call on the same window bit for bit.
    A non-causal call needs N <= M (for every sequence of a host table): a row with pos_i < 0 has no key at distance 0, so a steep slope
    could push its whole row under the static window.  Under causal with N > M, rows without a visible key give 0, as in every call.
    Table checks and max_seqlen rules of `flash_cosine_sim_attention_varlen`.  CPU tensors take the forward-only path of `cpu.py`."""
    window = _window(window_size)
    if not isinstance(alibi_slopes, torch.Tensor) or alibi_slopes.dtype != torch.float32:
        raise TypeError(f"alibi_slopes must be a float32 tensor of shape [heads] or [batch, heads], got "
                        f"{getattr(alibi_slopes, 'dtype', type(alibi_slopes).__name__)}")
    if alibi_slopes.requires_grad:
        raise ValueError("alibi_slopes must not require grad: there is no slope gradient (fixed slopes only)")
    packed, max_seqlen_q, max_seqlen_k = _dense_or_packed("flash_cosine_sim_attention_alibi", q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
                                                          max_seqlen_k)
    if packed:
        H, B = q.shape[1], cu_seqlens_q.numel() - 1
        if not causal and cu_seqlens_q.device.type == "cpu" and cu_seqlens_k.device.type == "cpu":
            nq, nk = cu_seqlens_q[1:] - cu_seqlens_q[:-1], cu_seqlens_k[1:] - cu_seqlens_k[:-1]
            if bool((nq > nk).any()):
                raise ValueError("alibi_slopes: a non-causal call needs N <= M for every sequence (rows with a negative position have no key "
                                 "at distance 0)")
    else:
        H, B = q.shape[1], q.shape[0]
        if not causal and q.shape[2] > k.shape[2]:
            raise ValueError(f"alibi_slopes: a non-causal call needs N <= M, got N = {q.shape[2]} > M = {k.shape[2]} (rows with a negative "
                             "position have no key at distance 0)")
    if tuple(alibi_slopes.shape) not in ((H,), (B, H)):
        raise ValueError(f"alibi_slopes must have shape [{H}] or [{B}, {H}] (heads, or {'sequences' if packed else 'batch'} x heads), got "
                         f"{tuple(alibi_slopes.shape)}")
    if alibi_slopes.device.type == "cpu":
        if not bool(torch.isfinite(alibi_slopes).all()) or bool((alibi_slopes < 0).any()):
            raise ValueError("alibi_slopes must be finite and >= 0 (the bias is a penalty)")
    elif alibi_slopes.device != q.device:
        raise ValueError(f"alibi_slopes is on {alibi_slopes.device} but q is on {q.device}")
    if q.device.type == "cpu":
        if alibi_slopes.device.type != "cpu":
            raise ValueError("CPU tensors take host alibi_slopes")
        if packed:
            return _cpu.attention_forward_varlen_cpu(q, k, v, cu_seqlens_q, cu_seqlens_k, scale=scale, groups=groups, causal=causal,
                                                     l2norm_qk=l2norm_qk, window_size=window, alibi_slopes=alibi_slopes)
        return _cpu.attention_forward_cpu(q, k, v, scale=scale, groups=groups, causal=causal, l2norm_qk=l2norm_qk, window_size=window,
                                          alibi_slopes=alibi_slopes)
    cu_q = cu_k = None
    max_q = max_k = 0
    if packed:
        cu_q, cu_k, max_q, max_k = _packed_on_device(q, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k)
    _torch_ops.load()
    return torch.ops.fcsa_alibi_train.attention(q, k, v, alibi_slopes.to(q.device, non_blocking=True), cu_q, cu_k, max_q, max_k, float(scale),
                                                bool(causal), bool(l2norm_qk), int(groups), window[0], window[1])


# ---------------------------------------------------------------------------------------------
# decoding against a key/value cache (flash-attn's kvcache convention; no reference counterpart)
# ---------------------------------------------------------------------------------------------

def _cache_scale(name, s, B, Hk, device):
    """k_scale / v_scale of an fp8 cache as a float32 tensor of shape [], [Hk] or [B, Hk] on `device`.  None: 1.0.  Values the host can
    see (a number, a host tensor) must be finite and > 0; a tensor already on a GPU is trusted, so the call does not synchronise."""
    if s is None:
        s = 1.0
    if isinstance(s, torch.Tensor):
        if s.dtype != torch.float32 or tuple(s.shape) not in ((), (Hk,), (B, Hk)):
            raise TypeError(f"{name} must be a float or a float32 tensor of shape [], [{Hk}] or [{B}, {Hk}], got {s.dtype} {tuple(s.shape)}")
        if s.device.type == "cpu" and not bool((torch.isfinite(s) & (s > 0)).all()):
            raise ValueError(f"{name} must be finite and > 0")
        return s.detach().to(device, non_blocking=True)
    if isinstance(s, bool) or not isinstance(s, (int, float)):
        raise TypeError(f"{name} must be a float or a float32 tensor, got {type(s).__name__}")
    if not (s > 0 and s != float("inf")):
        raise ValueError(f"{name} must be finite and > 0, got {s}")
    return torch.full((), float(s), dtype=torch.float32, device=device)


def _check_return_lse(return_lse):
    """return_lse sits where a positional window_size used to land (window_size stays the last parameter): anything but a bool is refused
    rather than read as a flag."""
    if not isinstance(return_lse, bool):
        raise TypeError(f"return_lse must be a bool, got {return_lse!r} (pass window_size by keyword)")


_FP8_TYPES = tuple(getattr(torch, n) for n in ("float8_e4m3fn", "float8_e4m3fnuz", "float8_e5m2", "float8_e5m2fnuz") if hasattr(torch, n))


def _host_view(q, cu_seqlens_q, k_new, cache_seqlens):
    """What the host can see of a decode step's per-sequence tables without reading a device tensor: (counts, lens, appended) -- the query
    rows, the cached positions and the positions this call appends, each a list with one entry per sequence, or None where the table
    lives on the device (lens also for cache_seqlens=None: every sequence full).  cu_seqlens_q None: a rectangular q [B, H, N, D].  It
    judges nothing: an argument it cannot read counts as unseen, and the checks of the cache functions refuse it."""
    host = lambda t: isinstance(t, torch.Tensor) and t.device.type == "cpu" and t.dim() == 1
    if cu_seqlens_q is None:
        B = q.shape[0]
        counts = [q.shape[2]] * B
        appended = [k_new.shape[2] if isinstance(k_new, torch.Tensor) and k_new.dim() == 4 else 0] * B
    else:
        B = cu_seqlens_q.numel() - 1 if isinstance(cu_seqlens_q, torch.Tensor) else 0
        counts = appended = None
        if host(cu_seqlens_q):
            c = cu_seqlens_q.tolist()
            counts = [hi - lo for lo, hi in zip(c[:-1], c[1:])]
            appended = counts if k_new is not None else [0] * B
    lens = None
    if isinstance(cache_seqlens, int):
        lens = [int(cache_seqlens)] * B
    elif host(cache_seqlens):
        lens = cache_seqlens.tolist()
    return counts, lens, appended


def _cache_capacity(k_cache, block_table, B, counted):
    """The positions per sequence of a cache that serves B sequences: contiguous [B, Hk, capacity, D], or paged by block_table (checked:
    int32 [B, max_blocks], pages a positive multiple of 16).  counted: whose B sequences the caches must match, for the message."""
    if block_table is None:
        if k_cache.shape[0] != B:
            raise ValueError(f"batch mismatch between {counted} ({B} sequences) and the caches ({k_cache.shape[0]})")
        return k_cache.shape[2]
    if not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.shape[0] != B:
        raise TypeError("block_table must be an int32 [sequences, max_blocks] tensor")
    page = k_cache.shape[2]
    if page <= 0 or page % 16:
        raise ValueError(f"page_size ({page}) must be a positive multiple of 16")
    return block_table.shape[1] * page


class _CacheCall:
    """The front end that every cache function shares, the equal-N one (`flash_cosine_sim_attention_with_kvcache`) and, through
    `_packed_call`, the packed ones (ragged, prefill, engine step, ALiBi, tree): the checks of the caches (here), of the tables, bounds and
    scales of a step of B sequences (`tables`), and the moves to q's device (`on_device`).  Nothing here reads a device tensor on the host."""

    def __init__(self, fn, q, q_fault, k_cache, v_cache, k_new, v_new, k_scale, v_scale):
        """q_fault: the caller's verdict on q's rank, None or the message to refuse it with (raised where the rank checks stand)."""
        self.q, self.k_cache, self.v_cache, self.k_new, self.k_scale, self.v_scale = q, k_cache, v_cache, k_new, k_scale, v_scale
        self.fp8 = k_cache.dtype in _FP8_TYPES or v_cache.dtype in _FP8_TYPES
        if self.fp8:
            if k_cache.dtype != v_cache.dtype:
                raise TypeError(f"one fp8 cache and one {min(k_cache.dtype, v_cache.dtype, key=lambda d: d in _FP8_TYPES)} cache: k_cache and "
                                f"v_cache must both be torch.float8_e4m3fn, got {k_cache.dtype} and {v_cache.dtype}")
            if k_cache.dtype != torch.float8_e4m3fn:
                raise TypeError(f"{k_cache.dtype} caches are not supported: an fp8 cache is torch.float8_e4m3fn (OCP e4m3, the gfx950 encoding; "
                                "float8_e4m3fnuz is MI300's, float8_e5m2 is out of scope)")
            if q.dtype not in (torch.float16, torch.bfloat16):
                raise TypeError(f"fp8 caches take float16 or bfloat16 q, k_new and v_new, got a {q.dtype} q")
            for name, t in (("k_new", k_new), ("v_new", v_new)):
                if t is not None and t.dtype != q.dtype:
                    raise TypeError(f"{name} must have q's dtype ({q.dtype}), got {t.dtype}")
        elif k_scale is not None or v_scale is not None:
            raise TypeError(f"k_scale / v_scale given with {k_cache.dtype} caches: scales belong to torch.float8_e4m3fn caches")
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (q, k_new, v_new)):
            raise RuntimeError(f"{fn} is forward-only: q, k_new and v_new must not require grad (run it under torch.no_grad())")
        if q_fault is not None:
            raise ValueError(q_fault)
        for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
            if t.dim() != 4:
                raise ValueError(f"{name} must have 4 dimensions, got {tuple(t.shape)}")
        if k_cache.shape != v_cache.shape:
            raise ValueError(f"k_cache and v_cache must have the same shape, got {tuple(k_cache.shape)} and {tuple(v_cache.shape)}")
        if (k_new is None) != (v_new is None):
            raise ValueError("k_new and v_new must be given together")
        H, self.Hk, self.D = q.shape[1], k_cache.shape[1], q.shape[-1]
        if k_cache.shape[3] != self.D:
            raise ValueError("query, key, value dimensions must be the same")
        if self.Hk < 1 or H % self.Hk:
            raise ValueError(f"k/v heads must divide q heads ({H}), got {self.Hk}")

    def tables(self, B, cu_seqlens_q, appends, cache_seqlens, block_table, max_seqlen_k):
        """The step's tables, checked: B sequences; cu_seqlens_q (checked by the caller) or None for a rectangular q; appends: whether
        k_new brings anything to append.  Sets capacity, max_k, the host's view (counts, lens, appended: `_host_view`) and the scales
        as tensors."""
        k_cache, page = self.k_cache, self.k_cache.shape[2]
        capacity = _cache_capacity(k_cache, block_table, B, "the step")
        if cache_seqlens is None:
            if appends:
                raise ValueError("k_new given but cache_seqlens is None (every sequence full): there is no slot to append to")
        elif not isinstance(cache_seqlens, int) and (not isinstance(cache_seqlens, torch.Tensor) or cache_seqlens.dtype != torch.int32
                                                     or cache_seqlens.shape != (B,)):
            raise TypeError(f"cache_seqlens must be an int or an int32 tensor of shape ({B},)")
        self.counts, self.lens, self.appended = _host_view(self.q, cu_seqlens_q, self.k_new, cache_seqlens)
        if self.lens is not None:
            ends = [n0 + n_new for n0, n_new in zip(self.lens, self.appended or [0] * B)]
            for b, (n0, end) in enumerate(zip(self.lens, ends)):
                if n0 < 0 or end > capacity:
                    raise ValueError(f"sequence {b}: cache_seqlens {n0} + {end - n0} new tokens outside [0, capacity {capacity}]")
            if block_table is not None and block_table.device.type == "cpu":
                nb = k_cache.shape[0]
                for b, end in enumerate(ends):
                    used = block_table[b, :(end + page - 1) // page]
                    if used.numel() and (int(used.min()) < 0 or int(used.max()) >= nb):
                        raise ValueError(f"sequence {b}: block_table entries outside [0, {nb})")
        if max_seqlen_k is not None and (int(max_seqlen_k) != max_seqlen_k or max_seqlen_k < 0):
            raise ValueError(f"max_seqlen_k must be a non-negative integer, got {max_seqlen_k}")
        if self.fp8:
            dev = self.q.device
            self.k_scale, self.v_scale = _cache_scale("k_scale", self.k_scale, B, self.Hk, dev), _cache_scale("v_scale", self.v_scale, B, self.Hk, dev)
        self.B, self.capacity = B, capacity
        self.max_k = capacity if max_seqlen_k is None else min(int(max_seqlen_k), capacity)
        self.cache_seqlens, self.block_table = cache_seqlens, block_table

    def cpu_quant(self):
        """the scale keywords of the CPU paths"""
        return dict(k_scale=self.k_scale.expand(self.B, self.Hk), v_scale=self.v_scale.expand(self.B, self.Hk)) if self.fp8 else {}

    def on_device(self):
        """(k_cache, v_cache, cache_seqlens, block_table) as the ops take them: the tables on q's device, and the codes of fp8 caches as
        bytes (same storage, so the append lands in the caller's caches)."""
        dev, cache_seqlens, block_table = self.q.device, self.cache_seqlens, self.block_table
        if isinstance(cache_seqlens, int):
            cache_seqlens = torch.full((self.B,), cache_seqlens, dtype=torch.int32, device=dev)
        elif cache_seqlens is not None:
            cache_seqlens = cache_seqlens.to(dev, non_blocking=True)
        if block_table is not None:
            block_table = block_table.to(dev, non_blocking=True)
        if self.fp8:
            return self.k_cache.view(torch.uint8), self.v_cache.view(torch.uint8), cache_seqlens, block_table
        return self.k_cache, self.v_cache, cache_seqlens, block_table


def flash_cosine_sim_attention_with_kvcache(q, k_cache, v_cache, k_new=None, v_new=None, cache_seqlens=None, block_table=None,
                                            max_seqlen_k=None, scale=8, groups=1, causal=False, l2norm_qk=True, k_scale=None, v_scale=None,
                                            return_lse=False, window_size=(-1, -1)):
    """Forward-only attention of new queries against a key/value cache, with an optional in-place append.

    q [B, H, N, D] (N = 1: plain decode; a few: speculative or chunked steps).  k_cache, v_cache: [B, Hk, capacity, D] or, with a
    block_table, paged [num_blocks, Hk, page_size, D] (page_size a multiple of 16); any strides with the feature dim contiguous, so a
    [B, capacity, Hk, D] (vLLM: [num_blocks, page_size, Hk, D]) buffer passed as .transpose(1, 2) works.  Hk divides H.
    block_table: int32 [B, max_blocks]; entry [b, i] is the block holding positions [i * page_size, (i + 1) * page_size) of sequence b.
    cache_seqlens: int32 [B] (device or host) or an int: tokens already cached per sequence; None: every sequence is full.
    k_new, v_new: [B, Hk, N_new, D], written into the cache at [cache_seqlens[b], cache_seqlens[b] + N_new) before attention reads it
    (cache_seqlens itself is not advanced).  With L_b = cache_seqlens[b] + N_new, o[b] equals flash_cosine_sim_attention(q[b:b+1], K_b,
    V_b, scale=, groups=, causal=, l2norm_qk=) over the first L_b cached positions (causal: bottom-right alignment; L_b == 0 gives 0).
    The cache holds raw keys; with l2norm_qk they are normalised as they are read.
    max_seqlen_k: an upper bound on every L_b that sizes the launch grid (default: the capacity), so the call never reads device tables
    on the host and a decode step can be captured in a HIP graph.  Host tables are validated; device tables are trusted (the kernels
    clamp lengths and block ids, so a malformed table gives wrong rows, never an access outside the tensors).  Two sequences appending
    into the same page slot is undefined behaviour.  CPU tensors take the forward-only path of `cpu.py`.
    window_size = (left, right): a sliding window -- the query at position t of its sequence sees the cached keys [t - left, t + right]
    (-1: unbounded; causal caps right at 0); only the cache blocks from the first visible key on are read.
    fp8 caches: when k_cache and v_cache are both torch.float8_e4m3fn (OCP e4m3; q, k_new, v_new float16 or bfloat16) they hold one-byte
    codes that mean k_scale[b, kvh] * code and v_scale[b, kvh] * code, and the result is what this function computes on those values.
    k_scale, v_scale: a Python float, or a float32 tensor of shape [], [Hk] or [B, Hk]; None is 1.0.  Host scales are checked to be finite
    and > 0; device tensors are trusted (and with device cache_seqlens and max_seqlen_k given the call does not synchronise).  The append
    quantises: code = e4m3_rne(clamp(float(x) / scale, -448, 448)), NaN stays NaN.  Choosing scales: for V the per-head amax / 448 uses
    the whole code range; for K under l2norm_qk the scale cancels (the keys are normalised as they are read), so any value that keeps
    K's codes in range serves -- amax / 448 again, or 1.0 for keys of ordinary size; without l2norm_qk choose it as for V.
    return_lse=True: returns (o, lse).  lse is float32 [B, H, N]: the natural log of the sum over the row's visible keys of exp(logit), the
    logit being scale * (sum over the groups of q^ . k^), or scale * q . k without l2norm_qk; with an fp8 cache k_scale is inside it and
    v_scale is not.  A row without a visible key has lse = -inf (and o = 0).  o and the caches are bit for bit those of the call without
    it.  (o, lse) is an attention state: `merge_attention_states` combines the states of the same queries over disjoint sets of keys.
    return_lse must be a bool and window_size is best passed by keyword: return_lse precedes it in the signature.
    Tree attention (a tree_mask over the step's tokens, for speculative decoding) is not taken here: pass cu_seqlens_q = arange(B + 1) * N
    and the packed q to `flash_cosine_sim_attention_tree_with_kvcache`, which takes one."""
    _check_return_lse(return_lse)
    window = _window(window_size)
    q_fault = None if q.dim() == 4 else f"q must have 4 dimensions, got {tuple(q.shape)}"
    c = _CacheCall("flash_cosine_sim_attention_with_kvcache", q, q_fault, k_cache, v_cache, k_new, v_new, k_scale, v_scale)
    B, H, N, D = q.shape
    if k_new is not None:
        if k_new.shape != v_new.shape or k_new.dim() != 4 or tuple(k_new.shape[:2]) != (B, c.Hk) or k_new.shape[3] != D:
            raise ValueError(f"k_new / v_new must be [{B}, {c.Hk}, N_new, {D}], got {tuple(k_new.shape)} and {tuple(v_new.shape)}")
    n_new = 0 if k_new is None else k_new.shape[2]
    c.tables(B, None, bool(n_new), cache_seqlens, block_table, max_seqlen_k)
    if q.device.type == "cpu":
        if cache_seqlens is not None and c.lens is None:
            raise ValueError("CPU tensors take host cache_seqlens")
        lens = c.lens if c.lens is not None else [c.capacity - n_new] * B
        detach = lambda t: None if t is None else t.detach()          # (grad mode is off here, or nothing requires grad)
        return _cpu.attention_forward_kvcache_cpu(q.detach(), k_cache, v_cache, detach(k_new), detach(v_new), lens, block_table,
                                                  scale=scale, groups=groups, causal=causal, l2norm_qk=l2norm_qk, window_size=window,
                                                  return_lse=bool(return_lse), **c.cpu_quant())
    k_cache, v_cache, cache_seqlens, block_table = c.on_device()
    tail = (float(scale), bool(causal), bool(l2norm_qk), int(groups))
    if return_lse:      # every route through one op: the same append and decode launches, a combine that also writes the lse
        return _torch_ops.load().kvcache_lse_forward(q, k_cache, v_cache, None, k_new, v_new, cache_seqlens, block_table, c.k_scale, c.v_scale, 0,
                                                     c.max_k, *tail, window[0], window[1])
    if c.fp8:
        return _torch_ops.load().kvcache_fp8_forward(q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, c.k_scale, c.v_scale, c.max_k,
                                                     *tail, window[0], window[1])
    if window != (-1, -1):
        return _torch_ops.load().kvcache_window_forward(q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, c.max_k, *tail,
                                                        window[0], window[1])
    return _torch_ops.load().kvcache_forward(q, k_cache, v_cache, k_new, v_new, cache_seqlens, block_table, c.max_k, *tail)


def _step_count(name, value):
    """chunk_rows / max_decode_tokens: None or a non-negative integer"""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, int):
        raise TypeError(f"{name} must be None or a non-negative integer, got {value!r}")
    if value < 0:
        raise ValueError(f"{name} must be None or a non-negative integer, got {value}")
    return value


def _step_routing(c, total_q, H, chunk_rows, max_decode_tokens):
    """The routing fields of an engine step, for every call that is one: (chunk_rows threshold, decode-rows bound, no_decode, no_chunk)"""
    threshold = _lib.STEP_CHUNK_ROWS if chunk_rows is None else min(chunk_rows, 2 ** 31 - 1)
    bound, no_decode, no_chunk = (-1 if max_decode_tokens is None else min(max_decode_tokens, total_q)), False, False
    if c.counts is not None:      # a host table: the decode-routed rows exactly, and which launch would find no sequence
        G = H // c.Hk
        decode = [n for n in c.counts if n > 0 and G * n < threshold]
        bound, no_decode, no_chunk = sum(decode), not decode, len(decode) == sum(1 for n in c.counts if n > 0)
    return threshold, bound, no_decode, no_chunk


def _empty_result(q, return_lse):
    """a packed step without rows: nothing to append, nothing to write, no launch"""
    o = q.new_empty(q.shape)
    return (o, q.new_empty((0, q.shape[1]), dtype=torch.float32)) if return_lse else o


def _step_arguments(return_lse, window_size, chunk_rows=None, max_decode_tokens=None):
    """The argument checks that open every packed cache function, before its own: returns (window, chunk_rows, max_decode_tokens)."""
    _check_return_lse(return_lse)
    return _window(window_size), _step_count("chunk_rows", chunk_rows), _step_count("max_decode_tokens", max_decode_tokens)


def _packed_call(fn, q, k_cache, v_cache, cu_seqlens_q, k_new, v_new, cache_seqlens, block_table, max_seqlen_q, max_seqlen_k, k_scale, v_scale,
                 *, return_lse, window, cpu_kw, op, routing=None, launch_empty=False):
    """What the packed cache functions share once their own arguments are checked: the checks of a packed step (q's rank, the caches,
    cu_seqlens_q, the packed new rows, the bounds, the tables); for CPU tensors the forward-only path of `cpu.py` with the keywords
    cpu_kw; the empty result of a step without rows (unless launch_empty); the moves to q's device; the op; and the choice of o or (o, lse).
    op(s) makes the function's op call and returns (o, lse).  s holds what the ops take beyond the function's own arguments: k_cache,
    v_cache, cache_seqlens, block_table (`_CacheCall.on_device`), cu_q, k_scale, v_scale, max_q, max_k and, with routing = (chunk_rows,
    max_decode_tokens), routing: the four fields of `_step_routing`."""
    q_fault = None if q.dim() == 3 else f"q must be a packed [total_q, heads, dim_head] tensor, got {tuple(q.shape)}"
    c = _CacheCall(fn, q, q_fault, k_cache, v_cache, k_new, v_new, k_scale, v_scale)
    if not isinstance(cu_seqlens_q, torch.Tensor) or cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1 or cu_seqlens_q.numel() < 1:
        raise TypeError("cu_seqlens_q must be a 1-D int32 tensor of sequences + 1 entries")
    total_q, H, D = q.shape
    B = cu_seqlens_q.numel() - 1
    if k_new is not None and (k_new.shape != v_new.shape or tuple(k_new.shape) != (total_q, c.Hk, D)):
        raise ValueError(f"k_new / v_new must be packed like q, [{total_q}, {c.Hk}, {D}], got {tuple(k_new.shape)} and {tuple(v_new.shape)}")
    if max_seqlen_q is not None and (int(max_seqlen_q) != max_seqlen_q or max_seqlen_q < 0):
        raise ValueError(f"max_seqlen_q must be a non-negative integer, got {max_seqlen_q}")
    if cu_seqlens_q.device.type == "cpu":
        _check_host_cu("cu_seqlens_q", cu_seqlens_q, total_q, None)
    c.tables(B, cu_seqlens_q, k_new is not None, cache_seqlens, block_table, max_seqlen_k)
    if q.device.type == "cpu":
        if c.counts is None or (cache_seqlens is not None and c.lens is None):
            raise ValueError("CPU tensors take host cu_seqlens_q and cache_seqlens tables")
        lens = c.lens if c.lens is not None else [c.capacity] * B
        detach = lambda t: None if t is None else t.detach()          # (grad mode is off here, or nothing requires grad)
        return _cpu.attention_forward_kvcache_varlen_cpu(q.detach(), k_cache, v_cache, cu_seqlens_q, detach(k_new), detach(v_new), lens, block_table,
                                                         window_size=window, return_lse=return_lse, **cpu_kw, **c.cpu_quant())
    max_q = total_q if max_seqlen_q is None else min(int(max_seqlen_q), total_q)
    cu_q = cu_seqlens_q.to(q.device, non_blocking=True)
    if total_q == 0 and not launch_empty:
        return _empty_result(q, return_lse)
    routing = None if routing is None else _step_routing(c, total_q, H, *routing)
    k_cache, v_cache, cache_seqlens, block_table = c.on_device()
    s = types.SimpleNamespace(k_cache=k_cache, v_cache=v_cache, cache_seqlens=cache_seqlens, block_table=block_table, cu_q=cu_q,
                              k_scale=c.k_scale, v_scale=c.v_scale, max_q=max_q, max_k=c.max_k, routing=routing)
    _torch_ops.load()
    o, lse = op(s)
    return (o, lse) if return_lse else o


def flash_cosine_sim_attention_varlen_with_kvcache(q, k_cache, v_cache, cu_seqlens_q, k_new=None, v_new=None, cache_seqlens=None,
                                                   block_table=None, max_seqlen_q=None, max_seqlen_k=None, scale=8, groups=1, causal=False,
                                                   l2norm_qk=True, k_scale=None, v_scale=None, return_lse=False, window_size=(-1, -1)):
    """A ragged decode step: `flash_cosine_sim_attention_with_kvcache` with a per-sequence number of queries, in one call.

    The step of a continuous-batching engine is never rectangular -- plain decodes bring 1 token, speculative sequences a few, a prompt
    chunk many.  q [total_q, H, D] packs the queries of B sequences back to back, as in `flash_cosine_sim_attention_varlen`: sequence b owns
    the rows [cu_seqlens_q[b], cu_seqlens_q[b + 1]) (int32 [B + 1]), N_b of them; N_b may be 0.  Returns o shaped like q.  Forward only.
    k_cache, v_cache, block_table, cache_seqlens, max_seqlen_k, k_scale / v_scale with float8_e4m3fn caches, window_size and every layout,
    stride and page rule are those of `flash_cosine_sim_attention_with_kvcache`.
    k_new, v_new: [total_q, Hk, D], packed by the same table -- every query token brings its key and value.  Sequence b's N_b rows are
    written at [cache_seqlens[b], cache_seqlens[b] + N_b) before attention reads the cache (slots at or beyond the capacity are dropped,
    cache_seqlens is not advanced, fp8 caches quantise as usual), and L_b = cache_seqlens[b] + N_b.  Without them L_b = cache_seqlens[b]
    (None: the capacity).
    Sequence b's rows equal `flash_cosine_sim_attention_with_kvcache` on that sequence alone (q_b [1, H, N_b, D], its own cache, the same
    keywords): causal is bottom-right aligned against L_b (query i sees keys j <= L_b - N_b + i), the window applies per sequence, rows
    without a visible key -- L_b == 0, or N_b > L_b under causal -- give 0.
    Host tables (cu_seqlens_q, cache_seqlens) are validated; device tables are trusted and clamped on the device, so a malformed table gives
    wrong rows, never an access outside the tensors.  max_seqlen_q (default total_q) and max_seqlen_k (default the capacity) are upper
    bounds that only size the launch: a wrong bound changes speed, never the result.  With device tables the call does not synchronise, so
    a step can be captured in a HIP graph.  CPU tensors take the forward-only path of `cpu.py` (host tables).
    The launch has one row-tile slot per 16 rows of G * N_b (about G * total_q / 16 + B per K/V head, whatever the longest sequence is), and
    every row tile re-reads and re-normalises its keys: this is the call for steps of one to a few dozen tokens per sequence.  Long prompt
    chunks work, at the decode kernel's efficiency; `flash_cosine_sim_attention_prefill_with_kvcache` is the call for those.
    return_lse=True: returns (o, lse) with lse float32 [total_q, H], as in `flash_cosine_sim_attention_with_kvcache`.
    Tree attention for speculative decoding (a tree_mask over the step's own tokens in place of causal) is this call under another name:
    `flash_cosine_sim_attention_tree_with_kvcache`, which takes these arguments and tree_mask."""
    window, _, _ = _step_arguments(return_lse, window_size)

    def op(s):      # the two ops take the same arguments; the one without the lse returns o alone
        args = (q, s.k_cache, s.v_cache, s.cu_q, k_new, v_new, s.cache_seqlens, s.block_table, s.k_scale, s.v_scale, s.max_q, s.max_k,
                float(scale), bool(causal), bool(l2norm_qk), int(groups), window[0], window[1])
        return torch.ops.fcsa.kvcache_lse_forward(*args) if return_lse else (torch.ops.fcsa.kvcache_varlen_forward(*args), None)
    return _packed_call("flash_cosine_sim_attention_varlen_with_kvcache", q, k_cache, v_cache, cu_seqlens_q, k_new, v_new, cache_seqlens,
                        block_table, max_seqlen_q, max_seqlen_k, k_scale, v_scale, return_lse=return_lse, window=window, op=op,
                        cpu_kw=dict(scale=scale, groups=groups, causal=causal, l2norm_qk=l2norm_qk), launch_empty=True)


def flash_cosine_sim_attention_prefill_with_kvcache(q, k_cache, v_cache, cu_seqlens_q, k_new=None, v_new=None, cache_seqlens=None,
                                                    block_table=None, max_seqlen_q=None, max_seqlen_k=None, scale=8, groups=1, causal=False,
                                                    l2norm_qk=True, k_scale=None, v_scale=None, return_lse=False, window_size=(-1, -1)):
    """Prompt chunks against the key/value cache: `flash_cosine_sim_attention_varlen_with_kvcache` on a kernel built for many rows per
    sequence.

    Arguments, layouts, the append of k_new / v_new before attention reads the cache, the per-sequence bottom-right causal alignment, o = 0
    and lse = -inf for rows without a visible key, N_b = 0, host tables validated and device tables trusted and clamped, no synchronisation
    with device tables (so the call can be captured in a HIP graph): all as in `flash_cosine_sim_attention_varlen_with_kvcache`, whose
    result this is -- bit for bit (o, lse and the caches) wherever that call runs one key split.
    The kernel: four waves own 128 token-major rows of one sequence's K/V head, share each 64-key stage of the cache through LDS and
    normalise every key once per workgroup (the ragged call: once per 16 rows); under causal a workgroup stops at its last visible key.
    There are NO key splits: the grid is about G * total_q / 128 + B workgroups per K/V head, so this is the call for chunks long enough to
    fill the chip with 128-row tiles (a few hundred tokens per sequence and up; max_seqlen_q and max_seqlen_k are accepted and size
    nothing).  Steps of one to a few dozen tokens per sequence belong to `flash_cosine_sim_attention_varlen_with_kvcache`.
    Supported: q, the caches and the new rows all float16 or all bfloat16; dim_head 64 or 128; any groups dividing it; any Hk dividing H.
    float32, float8_e4m3fn caches (k_scale / v_scale), other head dims and a window_size other than (-1, -1) are refused:
    `flash_cosine_sim_attention_varlen_with_kvcache` takes them.  CPU tensors are refused the same things and otherwise take the forward-only
    path of `cpu.py`.  Forward only.
    return_lse=True: returns (o, lse) with lse float32 [total_q, H]."""
    fn, other = "flash_cosine_sim_attention_prefill_with_kvcache", "flash_cosine_sim_attention_varlen_with_kvcache"
    window, _, _ = _step_arguments(return_lse, window_size)
    # what this kernel does not take, before anything else (and before the device branch: CPU tensors are refused the same things)
    if k_scale is not None or v_scale is not None or k_cache.dtype in _FP8_TYPES or v_cache.dtype in _FP8_TYPES:
        raise TypeError(f"{fn} does not take float8 caches or k_scale / v_scale: {other} takes them")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise TypeError(f"{fn} takes float16 or bfloat16 tensors, got {q.dtype}: {other} takes float32")
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache), ("k_new", k_new), ("v_new", v_new)):
        if t is not None and t.dtype != q.dtype:
            raise TypeError(f"{name} must have q's dtype ({q.dtype}), got {t.dtype}")
    if q.dim() == 3 and q.shape[-1] not in (64, 128):
        raise ValueError(f"{fn} takes head dimensions 64 and 128, got {q.shape[-1]}: {other} takes the others")
    if window != (-1, -1):
        raise ValueError(f"{fn} takes no sliding window (window_size {tuple(window_size)}): {other} takes one")
    op = lambda s: torch.ops.fcsa_prefill.kvcache_prefill_forward(q, s.k_cache, s.v_cache, s.cu_q, k_new, v_new, s.cache_seqlens, s.block_table,
                                                                  s.max_q, s.max_k, float(scale), bool(causal), bool(l2norm_qk), int(groups))
    return _packed_call(fn, q, k_cache, v_cache, cu_seqlens_q, k_new, v_new, cache_seqlens, block_table, max_seqlen_q, max_seqlen_k, None, None,
                        return_lse=return_lse, window=window, op=op, cpu_kw=dict(scale=scale, groups=groups, causal=causal, l2norm_qk=l2norm_qk))


def flash_cosine_sim_attention_step_with_kvcache(q, k_cache, v_cache, cu_seqlens_q, k_new=None, v_new=None, cache_seqlens=None,
                                                 block_table=None, max_seqlen_q=None, max_seqlen_k=None, scale=8, groups=1, causal=False,
                                                 l2norm_qk=True, k_scale=None, v_scale=None, return_lse=False, window_size=(-1, -1),
                                                 chunk_rows=None, max_decode_tokens=None):
    """The step of a continuous-batching engine against the key/value cache, in one call: a packed batch where most sequences bring one
    token, some a few and one or two a prompt chunk, each sequence sent to the kernel built for its row count.

    The two single-kernel calls are `flash_cosine_sim_attention_varlen_with_kvcache` (the ragged decode kernel: one wave per 16 rows, key
    splits) and `flash_cosine_sim_attention_prefill_with_kvcache` (the chunk kernel: 128 rows per workgroup, keys normalised once, no
    splits); each of them runs the whole batch on its one kernel.  This call takes the ragged call's arguments and returns the ragged call's
    result, and appends k_new / v_new once.
    Routing rule: sequence b, with N_b packed rows and G = H / Hk, takes the chunk kernel iff G * N_b >= chunk_rows and the decode kernel
    (with key splits) otherwise.  chunk_rows=None is the library default (1024: eight 128-row tiles); 0 sends every sequence to the chunk
    kernel, a value above G * total_q every sequence to the decode kernel.  Both kernels evaluate the rule on the device from the clamped
    table, so every row is written exactly once whatever a device table holds.
    Everything else -- arguments and layouts (contiguous or paged), float8_e4m3fn caches with k_scale / v_scale, window_size, the append,
    the per-sequence bottom-right causal alignment, o = 0 and lse = -inf for rows without a visible key, N_b = 0, host tables validated and
    device tables trusted and clamped, no synchronisation with device tables (so a step can be captured in a HIP graph), return_lse -- is
    as in `flash_cosine_sim_attention_varlen_with_kvcache`.  o, lse and both caches are that call's: a chunk-routed sequence's rows are bit
    for bit its rows at one key split, a decode-routed sequence's rows bit for bit its rows at this call's split count.
    max_decode_tokens: an upper bound on the packed rows of all decode-routed sequences (default total_q).  Like max_seqlen_q / max_seqlen_k
    it only sizes the split count: a wrong bound changes speed, never the result.  With a host cu_seqlens_q it is not needed: the count is
    taken from the table, and a launch that would find no sequence is skipped.  With a device table both launches always run.
    float32 tensors and head dimensions other than 64 and 128 have no chunk kernel: there this call is the ragged call (chunk_rows and
    max_decode_tokens are checked and otherwise ignored).  CPU tensors take the forward-only path of `cpu.py`.  Forward only."""
    window, chunk_rows, max_decode_tokens = _step_arguments(return_lse, window_size, chunk_rows, max_decode_tokens)
    op = lambda s: torch.ops.fcsa_step.kvcache_step_forward(q, s.k_cache, s.v_cache, s.cu_q, k_new, v_new, s.cache_seqlens, s.block_table,
                                                            s.k_scale, s.v_scale, s.max_q, s.max_k, float(scale), bool(causal), bool(l2norm_qk),
                                                            int(groups), window[0], window[1], *s.routing)
    return _packed_call("flash_cosine_sim_attention_step_with_kvcache", q, k_cache, v_cache, cu_seqlens_q, k_new, v_new, cache_seqlens,
                        block_table, max_seqlen_q, max_seqlen_k, k_scale, v_scale, return_lse=return_lse, window=window, op=op,
                        cpu_kw=dict(scale=scale, groups=groups, causal=causal, l2norm_qk=l2norm_qk), routing=(chunk_rows, max_decode_tokens))


def flash_cosine_sim_attention_alibi_with_kvcache(q, k_cache, v_cache, cu_seqlens_q, k_new=None, v_new=None, cache_seqlens=None,
                                                  block_table=None, max_seqlen_q=None, max_seqlen_k=None, scale=8, groups=1, causal=False,
                                                  l2norm_qk=True, k_scale=None, v_scale=None, return_lse=False, window_size=(-1, -1),
                                                  chunk_rows=None, max_decode_tokens=None, alibi_slopes=None):
    """A linear position bias (ALiBi) for the cached calls: `flash_cosine_sim_attention_step_with_kvcache` with one more, last keyword.
    The arguments are that call's, in its order; alibi_slopes=None IS that call, bit for bit, launching exactly what it launches.

    A model trained with a distance bias (`flash_cosine_sim_attention(..., attn_bias=-slope_h * |i - j|)`) is served through this call: a
    materialised [H, N, M] bias is no answer for a cache that grows every step, the linear form is one multiply-add per logit in registers.
    One function serves decode, prompt chunks and mixed steps: chunk_rows above G * total_q sends every sequence to the ragged decode kernel
    with key splits, chunk_rows=0 every sequence to the chunk kernel, the default routes each by its row count.  Equal-N users pass
    cu_seqlens_q = arange(B + 1) * N and the packed q.
    alibi_slopes: a float32 tensor [H] (every sequence) or [B, H].  With pos_i = L_b - N_b + i, the position of query i of sequence b (the
    bottom-right alignment of causal and of the window; L_b as the ragged call defines it), the logit of key j gains
    -alibi_slopes[b, h] * |pos_i - j|, in natural units after scale (with fp8 caches after k_scale), and is part of lse.  Any sign is
    allowed; non-causal calls bias the keys to the right by the absolute distance.  A host tensor is checked to be finite and moved to q's
    device without blocking; a device tensor is trusted and never read on the host, so the call does not synchronise and can be captured in
    a graph (slopes changed in place are picked up on replay).
    causal, window_size, paged / strided / float8_e4m3fn caches, return_lse, the append, N_b = 0 and rows without a visible key (o = 0,
    lse = -inf) combine with the bias exactly as in the step call.
    Numerics: the slopes are device data the host cannot bound and a negative slope gives a positive bias, so every call with slopes runs
    the per-row-shift regime (the online row maximum includes the bias) whatever dtype, scale and l2norm_qk say.  Zero slopes therefore
    equal the step call bit for bit only where that call runs the same regime (e.g. float16 at scale 16), and within rounding elsewhere.
    Not taken by: the tree call (a tree token's position is its depth, not its slot), the shared-prefix call (its prefix phase mixes
    sequences with different positions in one B = 1 call).  Training with the same bias: `flash_cosine_sim_attention_alibi`.  CPU tensors take the
    forward-only path of `cpu.py` (host slopes).  Forward only."""
    fn = "flash_cosine_sim_attention_alibi_with_kvcache"
    if alibi_slopes is None:
        return flash_cosine_sim_attention_step_with_kvcache(q, k_cache, v_cache, cu_seqlens_q, k_new, v_new, cache_seqlens, block_table, max_seqlen_q,
                                                            max_seqlen_k, scale, groups, causal, l2norm_qk, k_scale, v_scale, return_lse, window_size,
                                                            chunk_rows, max_decode_tokens)
    window, chunk_rows, max_decode_tokens = _step_arguments(return_lse, window_size, chunk_rows, max_decode_tokens)
    if not isinstance(alibi_slopes, torch.Tensor) or alibi_slopes.dtype != torch.float32:
        raise TypeError(f"alibi_slopes must be a float32 tensor of shape [heads] or [sequences, heads], got "
                        f"{getattr(alibi_slopes, 'dtype', type(alibi_slopes).__name__)}")
    if q.dim() == 3 and isinstance(cu_seqlens_q, torch.Tensor) and cu_seqlens_q.dim() == 1:
        H, B = q.shape[1], cu_seqlens_q.numel() - 1
        if tuple(alibi_slopes.shape) not in ((H,), (B, H)):
            raise ValueError(f"alibi_slopes must have shape [{H}] or [{B}, {H}] (heads, or sequences x heads), got {tuple(alibi_slopes.shape)}")
    if alibi_slopes.device.type == "cpu":
        if not bool(torch.isfinite(alibi_slopes).all()):
            raise ValueError("alibi_slopes must be finite")
    elif alibi_slopes.device != q.device:
        raise ValueError(f"alibi_slopes is on {alibi_slopes.device} but q is on {q.device}")
    if q.device.type == "cpu" and alibi_slopes.device.type != "cpu":
        raise ValueError("CPU tensors take host alibi_slopes")
    op = lambda s: torch.ops.fcsa_alibi.kvcache_alibi_forward(q, s.k_cache, s.v_cache, s.cu_q, alibi_slopes.detach().to(q.device, non_blocking=True),
                                                              k_new, v_new, s.cache_seqlens, s.block_table, s.k_scale, s.v_scale, s.max_q, s.max_k,
                                                              float(scale), bool(causal), bool(l2norm_qk), int(groups), window[0], window[1],
                                                              *s.routing)
    return _packed_call(fn, q, k_cache, v_cache, cu_seqlens_q, k_new, v_new, cache_seqlens, block_table, max_seqlen_q, max_seqlen_k, k_scale,
                        v_scale, return_lse=return_lse, window=window, op=op, routing=(chunk_rows, max_decode_tokens),
                        cpu_kw=dict(scale=scale, groups=groups, causal=causal, l2norm_qk=l2norm_qk, alibi_slopes=alibi_slopes.detach()))


def flash_cosine_sim_attention_tree_with_kvcache(q, k_cache, v_cache, cu_seqlens_q, k_new=None, v_new=None, cache_seqlens=None,
                                                 block_table=None, max_seqlen_q=None, max_seqlen_k=None, scale=8, groups=1, causal=False,
                                                 l2norm_qk=True, k_scale=None, v_scale=None, return_lse=False, window_size=(-1, -1),
                                                 tree_mask=None):
    """Tree attention for speculative decoding against the key/value cache: `flash_cosine_sim_attention_varlen_with_kvcache`
    with one more, last keyword.  The arguments are that call's, in its order; tree_mask=None IS that call, bit for bit, launching
    exactly what it launches.

    A speculative decoder (Medusa, EAGLE, SpecInfer, sequoia-style trees) drafts a tree of tokens per sequence and verifies it in one
    step: token t must see the cache, its ancestors and itself, but not its siblings or cousins, which sit in the same step; causal treats
    the step's tokens as a chain.
    tree_mask (tree attention for speculative decoding): an int64 tensor [total_q] on q's device, packed by cu_seqlens_q like q -- word
    tree_mask[cu_seqlens_q[b] + i] belongs to query i of sequence b -- that states which of the step's own tokens a query sees, in place
    of causal.  With L_b as the ragged call defines it (cache_seqlens[b] + N_b with an append, cache_seqlens[b] without) and
    P_b = L_b - N_b: every query of sequence b sees the cache positions j < P_b (everything before the
    step); query i sees position P_b + t, 0 <= t < N_b (the step's token t), iff bit t of its word is set (bit 0 the least significant,
    the word read as unsigned; bits t >= N_b are never looked at; positions below 0, N_b > L_b, do not exist).  A drafted tree sets, for
    token i, the bits of its ancestors and its own; but nothing requires a tree, the diagonal or a lower-triangular mask: a word is a
    per-row bit set over the step's tokens.  A sequence with N_b > 64 ignores its words and is causal, bottom-right, exactly as
    causal=True treats it (decided on the device from the clamped table), so a prompt chunk can ride in the same packed batch.  A row
    without a visible key gives o = 0 and lse = -inf.  causal=True or a window_size other than (-1, -1) with a mask: ValueError.  Everything
    else combines as without it: return_lse, fp8 caches, paged caches, k_new=None, device tables without synchronisation, graph capture
    (the mask is device data, never read by the host).  The launch is planned as the non-causal call on the same shapes and only the
    per-logit visibility test differs, so the chain mask (word i = bits 0 .. i) gives causal=True's o, lse and caches bit for bit, and
    all bits set give causal=False's.  After verification `kvcache_keep_accepted` moves the accepted path to the front of the step's
    slots.  The equal-N call takes no mask: pass cu_seqlens_q = arange(B + 1) * N here; the prefill, engine-step and shared-prefix
    calls take none either."""
    fn = "flash_cosine_sim_attention_tree_with_kvcache"
    if tree_mask is None:
        return flash_cosine_sim_attention_varlen_with_kvcache(q, k_cache, v_cache, cu_seqlens_q, k_new, v_new, cache_seqlens, block_table, max_seqlen_q,
                                                              max_seqlen_k, scale, groups, causal, l2norm_qk, k_scale, v_scale, return_lse, window_size)
    window, _, _ = _step_arguments(return_lse, window_size)
    if causal:
        raise ValueError("tree_mask states the visibility of the step's tokens: causal=True cannot be given with it")
    if window != (-1, -1):
        raise ValueError(f"tree_mask takes no sliding window (window_size {tuple(window_size)})")
    if not isinstance(tree_mask, torch.Tensor) or tree_mask.dtype != torch.int64:
        raise TypeError(f"tree_mask must be an int64 tensor of shape [total_q], got {getattr(tree_mask, 'dtype', type(tree_mask).__name__)}")
    if q.dim() == 3 and tuple(tree_mask.shape) != (q.shape[0],):
        raise ValueError(f"tree_mask must have shape [{q.shape[0]}] (one word per packed query row), got {tuple(tree_mask.shape)}")
    if tree_mask.device != q.device:
        raise ValueError(f"tree_mask is on {tree_mask.device} but q is on {q.device}")
    op = lambda s: torch.ops.fcsa_tree.kvcache_tree_forward(q, s.k_cache, s.v_cache, s.cu_q, tree_mask, k_new, v_new, s.cache_seqlens, s.block_table,
                                                            s.k_scale, s.v_scale, s.max_q, s.max_k, float(scale), bool(l2norm_qk), int(groups))
    return _packed_call(fn, q, k_cache, v_cache, cu_seqlens_q, k_new, v_new, cache_seqlens, block_table, max_seqlen_q, max_seqlen_k, k_scale,
                        v_scale, return_lse=return_lse, window=window, op=op,
                        cpu_kw=dict(scale=scale, groups=groups, l2norm_qk=l2norm_qk, tree_mask=tree_mask))


def kvcache_keep_accepted(k_cache, v_cache, cache_seqlens, accepted, num_accepted, block_table=None):
    """Moves the accepted path of a tree step to the front of the slots the step appended, in place.  Returns None.

    A tree step (`flash_cosine_sim_attention_tree_with_kvcache` with tree_mask and k_new / v_new) appends sequence b's N_b drafted tokens
    at [cache_seqlens[b], cache_seqlens[b] + N_b).  After verification the accepted tokens are a root-to-leaf path scattered over those
    slots; before the next step they must be its first num_accepted[b] slots.
    accepted: int32 [B, A], 1 <= A <= 64; num_accepted: int32 [B].  For i < num_accepted[b], accepted[b, i] is a step-token index in
    [0, 64), strictly increasing in i (so accepted[b, i] >= i); entries beyond num_accepted[b] are ignored.  The row at cache position
    cache_seqlens[b] + accepted[b, i] moves to cache_seqlens[b] + i, in K and in V, for every K/V head.  cache_seqlens (int32 [B]) is NOT
    advanced: the caller adds num_accepted.
    k_cache, v_cache, block_table: the layouts, strides and page rule of `flash_cosine_sim_attention_with_kvcache`.  Rows move as bytes,
    so every cache dtype works unchanged, float8_e4m3fn codes included (the scales are per sequence and K/V head).
    Host tables are validated (range, strict increase, num_accepted <= A, slots inside the capacity); device tables are trusted and
    clamped -- num_accepted to [0, A], indices to [0, 63] -- and a move whose source or destination is at or beyond the capacity is
    skipped, so nothing outside [cache_seqlens[b], cache_seqlens[b] + 64) of a sequence is ever written.  With device tables the call does
    not synchronise and can be captured in a HIP graph.  One workgroup owns all moves of a (sequence, K/V head) pair and reads every
    source row before it writes the first, so a destination that is another move's source (accepted = [1, 2, 3, ...]) is safe.
    CPU tensors take the path of `cpu.py` (host tables)."""
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{name} must be a tensor of 4 dimensions")
    if k_cache.shape != v_cache.shape or k_cache.dtype != v_cache.dtype or k_cache.device != v_cache.device:
        raise ValueError("k_cache and v_cache must have the same shape, dtype and device")
    if not isinstance(accepted, torch.Tensor) or accepted.dtype != torch.int32 or accepted.dim() != 2:
        raise TypeError("accepted must be an int32 [sequences, A] tensor")
    B, A = accepted.shape
    if not 1 <= A <= 64:
        raise ValueError(f"accepted must have 1 <= A <= 64 columns, got {A}")
    for name, t in (("num_accepted", num_accepted), ("cache_seqlens", cache_seqlens)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (B,):
            raise TypeError(f"{name} must be an int32 tensor of shape ({B},)")
    capacity = _cache_capacity(k_cache, block_table, B, "accepted")
    host = lambda t: t.device.type == "cpu"
    if host(num_accepted):
        counts = num_accepted.tolist()
        if any(n < 0 or n > A for n in counts):
            raise ValueError(f"num_accepted must lie in [0, {A}], got {counts}")
        if host(accepted):
            for b, n in enumerate(counts):
                path = accepted[b, :n].tolist()
                if any(t < 0 or t >= 64 for t in path) or any(y <= x for x, y in zip(path, path[1:])):
                    raise ValueError(f"sequence {b}: accepted must be strictly increasing step-token indices in [0, 64), got {path}")
    if host(cache_seqlens) and any(n < 0 or n > capacity for n in cache_seqlens.tolist()):
        raise ValueError(f"cache_seqlens must lie in [0, capacity {capacity}], got {cache_seqlens.tolist()}")
    dev = k_cache.device
    if dev.type == "cpu":
        if not (host(accepted) and host(num_accepted) and host(cache_seqlens)) or (block_table is not None and not host(block_table)):
            raise ValueError("CPU caches take host tables")
        _cpu.kvcache_keep_accepted_cpu(k_cache, v_cache, cache_seqlens.tolist(), accepted.tolist(), num_accepted.tolist(), block_table)
        return None
    if k_cache.dtype in _FP8_TYPES:      # the codes travel as bytes (same storage)
        k_cache, v_cache = k_cache.view(torch.uint8), v_cache.view(torch.uint8)
    move = lambda t: None if t is None else t.to(dev, non_blocking=True)
    _torch_ops.load()
    torch.ops.fcsa_tree.kvcache_compact(k_cache, v_cache, move(cache_seqlens), move(accepted), move(num_accepted), move(block_table))
    return None


# ---------------------------------------------------------------------------------------------
# attention states: merging the results of the same queries over disjoint sets of keys, and the shared-prefix decode step built on it
# ---------------------------------------------------------------------------------------------

MERGE_MAX_STATES = 8


def merge_attention_states(os, lses):
    """Merges S attention states (o_s, lse_s) of the same queries, each over its own set of keys, into the state over all the keys.

    os: a sequence of 1 <= S <= 8 tensors of one shape and dtype (float16, bfloat16 or float32), 4-D [..., D] or packed [total_q, H, D];
    the feature dim a multiple of 4 (float32) or 8 (16-bit); any strides with the feature dim contiguous and rows 16-byte aligned are read
    in place (other layouts are copied).  lses: the matching
    float32 tensors without the feature dim, any strides -- what `return_lse=True` of the cache calls returns.  Returns (o, lse), freshly
    allocated and contiguous.  Per row, in float32: M = max_s lse_s; w_s = exp(lse_s - M); W = sum_s w_s; o = (sum_s w_s * o_s) / W,
    rounded once; lse = M + log(W).  A state with lse_s = -inf (no visible key) contributes exactly nothing whatever its o_s holds, and
    when every state is empty o = 0 and lse = -inf.  Deterministic.  +inf or NaN LSEs are not supported.
    More than 8 states: merge in two steps (the result is a state again).  GPU tensors run one launch of the merge kernel; CPU tensors
    take the path of `cpu.py`.  Forward only."""
    os, lses = _check_states(os, lses)
    if torch.is_grad_enabled() and any(t.requires_grad for t in os + lses):
        raise RuntimeError("merge_attention_states is forward-only: run it under torch.no_grad()")
    if os[0].device.type == "cpu":
        return _cpu.merge_attention_states_cpu(os, lses)
    o, lse = _torch_ops.load().merge_states(os, lses)
    return o, lse


def _check_states(os, lses):
    """The argument checks of `merge_attention_states` and `merge_attention_states_with_grad`; returns (os, lses) as lists."""
    os, lses = list(os), list(lses)
    if not os or len(os) != len(lses):
        raise ValueError(f"merge_attention_states takes as many lses as os and at least one state, got {len(os)} and {len(lses)}")
    if len(os) > MERGE_MAX_STATES:
        raise ValueError(f"merge_attention_states merges at most {MERGE_MAX_STATES} states in one call, got {len(os)}: merge in two steps "
                         "(the result of a merge is a state again)")
    o0 = os[0]
    if not isinstance(o0, torch.Tensor) or o0.dim() not in (3, 4):
        raise ValueError("os must be 4-D [..., D] or packed 3-D [total_q, H, D] tensors")
    if o0.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"os must be float32, float16 or bfloat16, got {o0.dtype}")
    per16 = 16 // o0.element_size()                    # rows are whole 16-byte chunks: 4 float32 or 8 16-bit features
    if o0.shape[-1] < per16 or o0.shape[-1] % per16:
        raise ValueError(f"the feature dim must be a positive multiple of {per16} for {o0.dtype}, got {o0.shape[-1]}")
    for s, (o, l) in enumerate(zip(os, lses)):
        if not isinstance(o, torch.Tensor) or not isinstance(l, torch.Tensor):
            raise TypeError("os and lses must be tensors")
        if o.dtype != o0.dtype:
            raise TypeError(f"os must share a dtype, got {o0.dtype} and {o.dtype} (state {s})")
        if o.shape != o0.shape:
            raise ValueError(f"os must share a shape, got {tuple(o0.shape)} and {tuple(o.shape)} (state {s})")
        if l.dtype != torch.float32:
            raise TypeError(f"lses must be float32, got {l.dtype} (state {s})")
        if l.shape != o0.shape[:-1]:
            raise ValueError(f"lse {s} must have the shape of its o without the feature dim, {tuple(o0.shape[:-1])}, got {tuple(l.shape)}")
        if o.device != o0.device or l.device != o0.device:
            raise ValueError("os and lses must live on one device")
    return os, lses


# ---------------------------------------------------------------------------------------------
# attention states for training: the forward's log-sum-exp as a differentiable result, and a differentiable merge
# ---------------------------------------------------------------------------------------------

def flash_cosine_sim_attention_with_lse(q, k, v, scale=8, groups=1, causal=False, l2norm_qk=True, window_size=(-1, -1), cu_seqlens_q=None,
                                        cu_seqlens_k=None, max_seqlen_q=None, max_seqlen_k=None):
    """`flash_cosine_sim_attention` (4-D q, k, v), `flash_cosine_sim_attention_local` (with a window_size) or
    `flash_cosine_sim_attention_varlen` (packed 3-D q, k, v with cu_seqlens_q / cu_seqlens_k) returning (o, lse): an attention STATE, both
    parts differentiable w.r.t. q, k, v -- what context-parallel (ring) training, blockwise training over key chunks and loss terms on the
    log-partition need.  `merge_attention_states_with_grad` joins the states of the same queries over disjoint key sets.

    o is the o of the operator underneath, bit for bit, and with no gradient flowing into lse so are dq, dk, dv: the same kernels run.
    lse: float32 [B, H, N] (packed: [total_q, H]), the natural log of the sum over the row's visible keys of exp(logit), the logit being
    scale * (sum over the groups of q^ . k^), or scale * q . k without l2norm_qk.  It is read off the normaliser the forward saves:
    lse = ln 2 * (c2 - L) with L the log2 the backward kernels seed their logit accumulators with -- the same in both exponent regimes.
    A row without a visible key (no keys; causal with N > M; a window past the keys) has lse = -inf exactly and o = 0, and takes no
    gradient whatever its lse gradient holds.  Where the constant-shift clamp acts (a row whose every visible logit lies far below the
    shift) the value is ln(max(l, eps)) + shift: consistent with o (o * exp(lse) is the un-normalised sum), unlike the unclamped LSE of
    the cache calls.  Accuracy, 16-bit types: the forward's row sum adds the P~ values rounded to the type, so lse carries up to one unit
    roundoff of it (3.9e-3 bfloat16, 4.9e-4 float16) -- below what the rounding of the operands q^, k^ already does to the logits (2 u
    |scale| groups).  Where it would not be (l2norm_qk=False: the caller's q, k are the operands; or |scale| * groups < 1/2) the lse is
    read off a second, float32 forward of the same call instead: float32-accurate, at the price of that pass.  A gradient for lse costs one subtraction per row in the dQ kernel: dS = P (dP - (delta - dlse)).
    Every dtype, head dim, K/V grouping and scale of the operators underneath.  There is no mask and no attn_bias (a mask needs a
    per-batch emptiness rule: not supported with the lse).  Table checks and max_seqlen rules of `flash_cosine_sim_attention_varlen`.
    CPU tensors: forward only, like the other CPU paths."""
    window = _window(window_size)
    packed, max_seqlen_q, max_seqlen_k = _dense_or_packed("flash_cosine_sim_attention_with_lse", q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
                                                          max_seqlen_k)
    if q.device.type == "cpu":
        if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
            raise RuntimeError("flash_cosine_sim_attention_with_lse is forward-only on CPU tensors: run it under torch.no_grad()")
        return _cpu.attention_state_cpu(q, k, v, cu_seqlens_q, cu_seqlens_k, scale=scale, groups=groups, causal=causal, l2norm_qk=l2norm_qk,
                                        window_size=window)
    cu_q = cu_k = None
    max_q = max_k = 0
    if packed:
        cu_q, cu_k, max_q, max_k = _packed_on_device(q, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k)
    _torch_ops.load()
    return torch.ops.fcsa_state.attention_state(q, k, v, cu_q, cu_k, max_q, max_k, float(scale), bool(causal), bool(l2norm_qk), int(groups),
                                                window[0], window[1])


def merge_attention_states_with_grad(os, lses):
    """`merge_attention_states`, differentiable w.r.t. every o_s and lse_s: the same checks, and on GPU tensors the same forward kernel, bit
    for bit.  With a_s = w_s / W the merge weights: d o_s = a_s * do (rounded once) and d lse_s = a_s * (dlse + <do, o_s> - sum_t a_t
    <do, o_t>), one launch of the merge backward kernel (float32 dot products reduced inside a wave: deterministic).  A state of weight 0
    (lse_s = -inf) gets zero gradients and its o_s is never read.  CPU tensors: `cpu.merge_attention_states_cpu`, which torch autograd
    differentiates."""
    os, lses = _check_states(os, lses)
    if os[0].device.type == "cpu":
        return _cpu.merge_attention_states_cpu(os, lses)
    _torch_ops.load()
    o, lse = torch.ops.fcsa_state.merge_state(os, lses)
    return o, lse


def flash_cosine_sim_attention_with_shared_prefix(q, prefix_k_cache, prefix_v_cache, k_cache, v_cache, prefix_len=None, prefix_block_table=None,
                                                  cu_seqlens_q=None, k_new=None, v_new=None, cache_seqlens=None, block_table=None,
                                                  max_seqlen_q=None, max_seqlen_k=None, scale=8, groups=1, causal=False, l2norm_qk=True,
                                                  k_scale=None, v_scale=None, prefix_k_scale=None, prefix_v_scale=None, return_lse=False,
                                                  window_size=(-1, -1)):
    """A decode step of a batch whose sequences share a prefix (a system prompt) that is cached ONCE ("cascade" decoding).

    Every sequence's keys are the P = prefix_len shared positions followed by its own L_b cached positions (after the append), and its
    queries are the last N_b of those P + L_b positions.  The result is what `flash_cosine_sim_attention_with_kvcache` gives on caches that
    each hold a copy of the prefix in front of the sequence's own positions -- or, with cu_seqlens_q (q packed [total_q, H, D]), what
    `flash_cosine_sim_attention_varlen_with_kvcache` gives -- without the copies, and with every prefix byte read and normalised once per
    16 query rows of the whole BATCH instead of once per sequence.
    It is three phases of existing pieces: the prefix phase, one B = 1 cache call over all the batch's query rows as one sequence
    (non-causal: every prefix key precedes every query); the suffix phase, the ordinary call on the per-sequence caches, append included;
    and one `merge_attention_states` of the two (o, lse) pairs, which reads the prefix phase's result through strided views in place.
    prefix_k_cache, prefix_v_cache: what a B = 1 cache call takes: [1, Hk, capacity, D], or a paged pool [num_blocks, Hk, page_size, D]
    with prefix_block_table int32 [1, n] -- the pool may be the very tensors passed as k_cache / v_cache.  Nothing is ever appended to the
    prefix.  prefix_len: an int, or a one-element int32 tensor (device: the call does not read it on the host); None: the whole prefix
    capacity.  P == 0 (known on the host) returns the suffix call's result bit for bit.  fp8 prefix caches take prefix_k_scale /
    prefix_v_scale (a float, or float32 of shape [] or [Hk]).
    q, k_cache, v_cache, cu_seqlens_q, k_new, v_new, cache_seqlens, block_table, max_seqlen_q, max_seqlen_k, scale, groups, causal,
    l2norm_qk, k_scale, v_scale: those of the two cache functions, for the sequences' own caches; cache_seqlens counts own positions only.
    causal is bottom-right against P + L_b.  It requires N_b <= L_b + 1 for every sequence: every query sits behind the prefix, as it does
    whenever the step's tokens are appended in this call (k_new) or were before (N_b = L_b + 1: the first query sees the prefix alone).  A
    query placed INSIDE the prefix would need a causal cut of the prefix that the one-sequence prefix phase cannot express; host tables are
    checked for it, device tables are trusted (such a row would see the whole prefix).
    window_size other than (-1, -1) raises ValueError: a window that reaches into the prefix needs a per-sequence alignment against P +
    L_b that the B = 1 prefix call cannot express.
    With a device prefix_len, device tables and max_seqlen_k given, the call does not synchronise and can be captured in a HIP graph; all
    launches go to the current stream, one after another.  Returns o shaped like q, or (o, lse) with return_lse=True.  Forward only.
    Tree attention (a tree_mask over the step's tokens) is not taken here: `flash_cosine_sim_attention_tree_with_kvcache` takes one."""
    _check_return_lse(return_lse)
    if _window(window_size) != (-1, -1):
        raise ValueError("flash_cosine_sim_attention_with_shared_prefix takes no window_size: a window that reaches into the shared prefix "
                         "needs a per-sequence alignment against prefix_len + L_b, which the single B = 1 prefix call cannot express")
    ragged = cu_seqlens_q is not None
    for name, t in (("prefix_k_cache", prefix_k_cache), ("prefix_v_cache", prefix_v_cache)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{name} must be a 4-D tensor ([1, Hk, capacity, D], or a paged pool with prefix_block_table)")
    if prefix_block_table is not None:
        if not isinstance(prefix_block_table, torch.Tensor) or prefix_block_table.dtype != torch.int32 or prefix_block_table.dim() != 2 \
                or prefix_block_table.shape[0] != 1:
            raise TypeError("prefix_block_table must be an int32 [1, n] tensor")
        prefix_cap = prefix_block_table.shape[1] * prefix_k_cache.shape[2]
    else:
        if prefix_k_cache.shape[0] != 1:
            raise ValueError(f"the shared prefix is one sequence: prefix_k_cache must be [1, Hk, capacity, D], got {tuple(prefix_k_cache.shape)}")
        prefix_cap = prefix_k_cache.shape[2]
    if q.dim() != (3 if ragged else 4):
        raise ValueError("q must be [B, H, N, D], or packed [total_q, H, D] with cu_seqlens_q")
    if prefix_len is None:
        plen = prefix_cap
    elif isinstance(prefix_len, torch.Tensor):
        if prefix_len.dtype != torch.int32 or prefix_len.numel() != 1:
            raise TypeError("prefix_len must be an int or a one-element int32 tensor")
        plen = int(prefix_len.item()) if prefix_len.device.type == "cpu" else prefix_len.reshape(1)
    elif isinstance(prefix_len, bool) or not isinstance(prefix_len, int):
        raise TypeError("prefix_len must be an int or a one-element int32 tensor")
    else:
        plen = prefix_len
    if isinstance(plen, int) and not 0 <= plen <= prefix_cap:
        raise ValueError(f"prefix_len {plen} outside [0, prefix capacity {prefix_cap}]")
    if causal:      # N_b <= L_b + 1 with L_b = cached + appended, as far as the host can see the tables
        counts, lens, appended = _host_view(q, cu_seqlens_q, k_new, cache_seqlens)
        if counts is not None and cache_seqlens is None and k_cache.dim() == 4:      # every sequence full
            lens = [block_table.shape[1] * k_cache.shape[2] if isinstance(block_table, torch.Tensor) and block_table.dim() == 2
                    else k_cache.shape[2]] * len(counts)
        if counts is not None and lens is not None and any(n > length + new + 1 for n, length, new in zip(counts, lens, appended)):
            raise ValueError("causal with a shared prefix needs every query behind the prefix (N_b <= L_b + 1, L_b counting this call's "
                             "append): a query placed inside the prefix needs a causal cut that the one-sequence prefix phase cannot express")
    own = dict(k_new=k_new, v_new=v_new, cache_seqlens=cache_seqlens, block_table=block_table, max_seqlen_k=max_seqlen_k, scale=scale,
               groups=groups, causal=causal, l2norm_qk=l2norm_qk, k_scale=k_scale, v_scale=v_scale, return_lse=True)
    # suffix phase: the ordinary call (every check of its arguments, and the append)
    if ragged:
        o_s, lse_s = flash_cosine_sim_attention_varlen_with_kvcache(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q=max_seqlen_q, **own)
    else:
        o_s, lse_s = flash_cosine_sim_attention_with_kvcache(q, k_cache, v_cache, **own)
    rows = q.shape[0] if ragged else q.shape[0] * q.shape[2]
    if (isinstance(plen, int) and plen == 0) or rows == 0 or q.shape[1] == 0:
        return (o_s, lse_s) if return_lse else o_s
    # prefix phase: all the batch's query rows as ONE sequence [1, H, rows, D] -- packed q is a transposed view, rectangular q one small copy
    H, D = q.shape[1], q.shape[-1]
    q1 = q.transpose(0, 1).unsqueeze(0) if ragged else q.transpose(0, 1).reshape(1, H, rows, D)
    o_p, lse_p = flash_cosine_sim_attention_with_kvcache(q1, prefix_k_cache, prefix_v_cache, cache_seqlens=plen, block_table=prefix_block_table,
                                                         scale=scale, groups=groups, causal=False, l2norm_qk=l2norm_qk,
                                                         k_scale=prefix_k_scale, v_scale=prefix_v_scale, return_lse=True)
    if ragged:
        o_pv, lse_pv = o_p[0].transpose(0, 1), lse_p[0].transpose(0, 1)                       # [total_q, H, D], [total_q, H]
    else:
        B, N = q.shape[0], q.shape[2]
        o_pv, lse_pv = o_p[0].view(H, B, N, D).transpose(0, 1), lse_p[0].view(H, B, N).transpose(0, 1)
    o, lse = merge_attention_states([o_pv, o_s], [lse_pv, lse_s])
    return (o, lse) if return_lse else o
