"""CPU-tensor behaviour of `flash_cosine_sim_attention` -- the operator's forward-only host path.

The reference dispatches non-CUDA tensors to a tiled pure-PyTorch forward
(flash_cosine_sim_attention.py:322-323 -> py:130-241) that never materialises the N x M logits and
refuses inputs that require gradients (py:142-144).  This module is this package's own version
of that path, so that callers which feed CPU tensors keep working:

  * blockwise accumulation of the un-normalised pair (P~ V, rowsum P~) with a CONSTANT exponent shift --
    the logits are bounded by scale * groups because q, k are l2-normalised, so no running max and no
    rescaling is needed (same algebra as the GPU kernels);
  * the key range of a row block is clipped to what causality allows BEFORE looping over key blocks, so
    blocks above the diagonal are never touched (the reference's own skip test, py:215, is inverted --
    it is wrong for causal N > 512, see DESIGN.md "Known reference defect");
  * float32 arithmetic inside, result cast back to the input dtype (py:147, py:241);
  * rows without any valid key come out as 0 (kernel semantics).

It is NOT a fallback for GPU tensors: those only ever run on the HIP kernels (`ops.py`), and a missing
libfcsa_hip.so raises.  Nothing here imports `oracle/` (test infrastructure).
"""
from __future__ import annotations

import torch


def normalise_groups(t: torch.Tensor, groups: int = 1) -> torch.Tensor:
    """Grouped l2norm over the last dim with the reference's CPU clamp (py:38-42: 1e-12 for float32, 1e-3 for the
    16-bit types), computed in float32 and rounded back to t's dtype (py:63-64)."""
    d = t.shape[-1]
    if groups < 1 or d % groups:
        raise ValueError(f"groups ({groups}) must divide the head dimension ({d})")
    floor = 1e-12 if t.dtype == torch.float32 else 1e-3
    g = t.float().reshape(*t.shape[:-1], groups, d // groups)
    length = torch.linalg.vector_norm(g, dim=-1, keepdim=True)
    return (g / length.clamp_min(floor)).reshape(t.shape).to(t.dtype)


def expand_kv_heads(t: torch.Tensor, heads: int) -> torch.Tensor:
    """K or V of shape [B, Hk, M, D] for `heads` query heads.  Hk == heads and Hk == 1 (single-headed: broadcast) are returned as
    they are; grouped-query K/V (1 < Hk < heads, heads % Hk == 0) is repeated so that query head h reads K/V head h // (heads // Hk),
    the repeat_interleave convention of torch's scaled_dot_product_attention(enable_gqa=True)."""
    hk = t.shape[1]
    if hk == heads or hk == 1:
        return t
    if hk < 1 or heads % hk:
        raise ValueError(f"k/v heads must divide q heads ({heads}): grouped-query attention needs H % Hk == 0, got Hk = {hk}")
    return t.repeat_interleave(heads // hk, dim=1)


def window_sides(window_size, causal):
    """(left, right) of a sliding window as the loops below use them: None for an unbounded side, `causal` caps right at 0."""
    left, right = window_index(window_size)
    return (None if left < 0 else left), (0 if causal else None if right < 0 else right)


def window_index(window_size):
    """(left, right) of a window_size argument as two Python ints >= -1: any integer type (operator.index), no bool, no float."""
    import operator
    try:
        left, right = window_size
    except (TypeError, ValueError):
        raise ValueError(f"window_size must be a pair (left, right), got {window_size!r}") from None
    out = []
    for side in (left, right):
        if isinstance(side, bool):
            raise ValueError(f"window_size sides must be integers, got {window_size!r}")
        try:
            side = operator.index(side)
        except TypeError:
            raise ValueError(f"window_size sides must be integers, got {window_size!r}") from None
        if side < -1:
            raise ValueError(f"window_size sides must be >= 0, or -1 for unbounded, got {window_size!r}")
        out.append(side)
    return tuple(out)


def attention_forward_cpu(q, k, v, mask=None, attn_bias=None, scale=8.0, groups=1, causal=False, l2norm_qk=True,
                          attn_bias_batch_dim=False, row_block=256, key_block=1024, window_size=(-1, -1), return_lse=False, tail_mask=None,
                          alibi_slopes=None):
    """Forward-only blockwise cosine-sim attention on host tensors.  Same argument meaning as the GPU operator.
    window_size = (left, right): query i sees key j iff i + (M - N) - left <= j <= i + (M - N) + right (-1: unbounded; causal caps
    right at 0); the key blocks outside a row block's band are never touched.
    return_lse: also return the rows' log-sum-exp, float32 of q's shape without the feature dim: log(sum over the visible keys of
    exp(logit)), from the running max and row sum the loop holds; -inf for a row without a visible key.
    tail_mask: bool [N, T], T <= M (a tree step, `tree_tail`): query i sees every key before the last T and key M - T + t iff tail_mask[i, t].
    It takes no causal, window, mask or bias.  A row block stops at the last key any of its rows sees, as a causal one does, and an
    invisible logit is -inf either way, so a lower-triangular mask gives the causal call's bits and a full one the plain call's.
    alibi_slopes: float32 [H], or [B, H] (the linear position bias of the cached calls and of `flash_cosine_sim_attention_alibi`): the logit of key j for query i gains -slope[h] * |i + (M - N) - j|
    after the scale, and is part of the lse.  It is computed per block, never materialised, and -- unlike attn_bias -- combines with a
    window; it takes no tail_mask and no attn_bias."""
    w_left, w_right = window_sides(window_size, causal)
    if alibi_slopes is not None and (tail_mask is not None or attn_bias is not None):
        raise ValueError("alibi_slopes takes no tail_mask and no attn_bias")
    if tail_mask is not None and (causal or mask is not None or attn_bias is not None or tuple(window_index(window_size)) != (-1, -1)):
        raise ValueError("tail_mask states the visibility: no causal, window_size, mask or attn_bias with it")
    if tuple(window_index(window_size)) != (-1, -1) and (mask is not None or attn_bias is not None):      # (as the C ABI: any window)
        raise ValueError("a sliding window takes no mask and no attn_bias")
    for name, t in (("q", q), ("k", k), ("v", v), ("attn_bias", attn_bias)):
        if t is not None and t.requires_grad:
            raise RuntimeError(f"{name} requires grad: the CPU path of flash_cosine_sim_attention is forward-only "
                               "(like the reference's, flash_cosine_sim_attention.py:142-144)")
    if causal and mask is not None:
        raise ValueError("mask should not be supplied if causality is needed")
    out_dtype, out_shape = q.dtype, q.shape
    merged = q.dim() == 3
    if merged:
        if k.dim() != 3 or v.dim() != 3:
            raise ValueError("if batch and heads are merged for queries, keys and values must also have 3 dimensions")
        attn_bias_batch_dim = True
        q = q.unsqueeze(1)
    if q.dim() != 4:
        raise ValueError(f"q must have 3 or 4 dimensions, got {q.dim()}")
    if l2norm_qk:
        q, k = normalise_groups(q, groups), normalise_groups(k, groups)
    B, H, N, D = q.shape
    # [B, 1 or H, M, D]: single-headed K/V broadcast over heads, grouped-query K/V repeated over each group
    k4 = expand_kv_heads(k.unsqueeze(1) if k.dim() == 3 else k, H)
    v4 = expand_kv_heads(v.unsqueeze(1) if v.dim() == 3 else v, H)
    M = k4.shape[2]
    qf, kt, vf = q.float(), k4.float().transpose(-1, -2), v4.float()
    bias = None
    if attn_bias is not None:
        bias = attn_bias.float().unsqueeze(1 if attn_bias_batch_dim else 0)          # [B,1,N,M] or [1,H,N,M]
    keep_keys = None if mask is None else mask.to(torch.bool)[:, None, None, :]      # [B,1,1,M]
    offset = M - N                                        # key j is visible to query i iff j <= i + offset (cu:1210)

    # Running row max with rescale (the exponent shift of a row is its own largest visible logit so far): exact for ANY scale,
    # groups, bias and for unnormalised q, k (l2norm_qk=False) -- a constant shift of scale * groups underflows whole rows to 0 once
    # scale * groups is large, and overflows without the l2norm.
    acc = torch.zeros((B, H, N, D), dtype=torch.float32)
    total = torch.zeros((B, H, N, 1), dtype=torch.float32)
    top = torch.full((B, H, N, 1), float("-inf"), dtype=torch.float32)
    for r0 in range(0, N, row_block):
        r1 = min(N, r0 + row_block)
        last = M if w_right is None else min(M, r1 + offset + w_right)      # keys >= last are invisible to every row of this block
        first = 0 if w_left is None else min(max(r0 + offset - w_left, 0), max(last, 0))     # ... and so are keys < first
        if tail_mask is not None:
            tail0 = M - tail_mask.shape[1]
            cols = tail_mask[r0:r1].any(dim=0).nonzero()
            last = tail0 + (int(cols.max()) + 1 if cols.numel() else 0)
        rows = qf[:, :, r0:r1]
        a, s, t = acc[:, :, r0:r1], total[:, :, r0:r1], top[:, :, r0:r1]
        for c0 in range(first, max(last, 0), key_block):
            c1 = min(last, c0 + key_block)
            logits = torch.matmul(rows, kt[..., c0:c1]) * scale
            if bias is not None:
                logits = logits + bias[:, :, r0:r1, c0:c1]
            visible = None
            ii = torch.arange(r0, r1).unsqueeze(1) + offset
            jj = torch.arange(c0, c1).unsqueeze(0)
            if alibi_slopes is not None:
                slopes = alibi_slopes.float()
                slopes = slopes.reshape(1, -1, 1, 1) if slopes.dim() == 1 else slopes.reshape(slopes.shape[0], slopes.shape[1], 1, 1)
                logits = logits - slopes * (ii - jj).abs().float()
            if w_right is not None and c1 - 1 > r0 + offset + w_right:           # the block touches the (right) diagonal
                visible = (jj <= ii + w_right)
            if w_left is not None and c0 < r1 - 1 + offset - w_left:              # ... the window's left edge
                inside = (jj >= ii - w_left)
                visible = inside if visible is None else (visible & inside)
            if keep_keys is not None:
                visible = keep_keys[..., c0:c1] if visible is None else (visible & keep_keys[..., c0:c1])
            if tail_mask is not None and c1 > tail0:
                visible = torch.ones((r1 - r0, c1 - c0), dtype=torch.bool)
                visible[:, max(c0, tail0) - c0:] = tail_mask[r0:r1, max(c0, tail0) - tail0:c1 - tail0]
            if visible is not None:
                logits = logits.masked_fill(~visible, float("-inf"))
            t_new = torch.maximum(t, logits.amax(dim=-1, keepdim=True))
            safe = torch.where(torch.isinf(t_new), torch.zeros_like(t_new), t_new)      # rows that have seen no key yet
            w = torch.exp(logits - safe)
            rescale = torch.exp(torch.where(torch.isinf(t), torch.zeros_like(t), t) - safe)
            a.mul_(rescale)
            s.mul_(rescale)
            a += torch.matmul(w, vf[:, :, c0:c1])
            s += w.sum(dim=-1, keepdim=True)
            t.copy_(t_new)
    out = acc / total.clamp_min(1e-30)                    # rows without a valid key: 0 / tiny = 0
    out = out.reshape(out_shape).to(out_dtype)
    if not return_lse:
        return out
    seen = total > 0                                      # (a row that saw no key has top = -inf and total = 0)
    lse = torch.where(seen, top + torch.log(torch.where(seen, total, torch.ones_like(total))), torch.full_like(top, float("-inf")))
    return out, lse.reshape(out_shape[:-1])


def attention_forward_varlen_cpu(q, k, v, cu_seqlens_q, cu_seqlens_k, scale=8.0, groups=1, causal=False, l2norm_qk=True,
                                 window_size=(-1, -1), alibi_slopes=None):
    """Forward-only path of `flash_cosine_sim_attention_varlen` on host tensors: packed q [total_q, H, D], k / v [total_k, Hk, D] and
    validated host tables; each sequence runs through `attention_forward_cpu` as a batch-1 problem, so its rows are exactly what the
    dense CPU path gives for that sequence alone.  alibi_slopes: float32 [H] or [sequences, H], per sequence as in `attention_forward_cpu`."""
    out = torch.zeros_like(q)
    cq, ck = cu_seqlens_q.tolist(), cu_seqlens_k.tolist()
    for s in range(len(cq) - 1):
        qs = q[cq[s]:cq[s + 1]].permute(1, 0, 2).unsqueeze(0)         # [1, H, N_s, D]
        ks = k[ck[s]:ck[s + 1]].permute(1, 0, 2).unsqueeze(0)
        vs = v[ck[s]:ck[s + 1]].permute(1, 0, 2).unsqueeze(0)
        if qs.shape[2] == 0:
            continue
        slopes = None if alibi_slopes is None else (alibi_slopes if alibi_slopes.dim() == 1 else alibi_slopes[s])
        o = attention_forward_cpu(qs, ks, vs, scale=scale, groups=groups, causal=causal, l2norm_qk=l2norm_qk, window_size=window_size,
                                  alibi_slopes=slopes)
        out[cq[s]:cq[s + 1]] = o[0].permute(1, 0, 2)
    return out


def attention_state_cpu(q, k, v, cu_seqlens_q=None, cu_seqlens_k=None, scale=8.0, groups=1, causal=False, l2norm_qk=True,
                        window_size=(-1, -1)):
    """Forward-only path of `flash_cosine_sim_attention_with_lse` on host tensors: (o, lse) of the dense / local call (4-D q, k, v; lse
    float32 [B, H, N]) or, with validated host tables, of the packed call (lse [total_q, H]), each sequence as a batch-1 problem.  o is
    what `attention_forward_cpu` / `attention_forward_varlen_cpu` give; lse = -inf for a row without a visible key."""
    kw = dict(scale=scale, groups=groups, causal=causal, l2norm_qk=l2norm_qk, window_size=window_size, return_lse=True)
    if cu_seqlens_q is None:
        return attention_forward_cpu(q.detach(), k.detach(), v.detach(), **kw)
    out = torch.zeros_like(q)
    lse = torch.full(q.shape[:-1], float("-inf"), dtype=torch.float32)
    cq, ck = cu_seqlens_q.tolist(), cu_seqlens_k.tolist()
    for s in range(len(cq) - 1):
        if cq[s + 1] == cq[s]:
            continue
        qs, ks, vs = (t.detach()[lo:hi].permute(1, 0, 2).unsqueeze(0) for t, lo, hi in ((q, cq[s], cq[s + 1]), (k, ck[s], ck[s + 1]),
                                                                                       (v, ck[s], ck[s + 1])))
        o, l = attention_forward_cpu(qs, ks, vs, **kw)
        out[cq[s]:cq[s + 1]] = o[0].permute(1, 0, 2)
        lse[cq[s]:cq[s + 1]] = l[0].permute(1, 0)
    return out, lse


def cache_gather(cache, b, length, block_table=None):
    """Positions [0, length) of sequence b of a key or value cache: [1, Hk, length, D].  Contiguous caches are [B, Hk, capacity, D]; paged
    ones [num_blocks, Hk, page_size, D] with block_table[b, i] holding positions [i * page_size, (i + 1) * page_size)."""
    if block_table is None:
        return cache[b:b + 1, :, :length]
    page = cache.shape[2]
    blocks = [int(x) for x in block_table[b, :(length + page - 1) // page].tolist()]
    if not blocks:
        return cache[:1, :, :0]
    return torch.cat([cache[i] for i in blocks], dim=1)[None, :, :length]


def append_kvcache_cpu(k_cache, v_cache, k_new, v_new, seqlens, block_table=None):
    """Writes k_new[b], v_new[b] ([B, Hk, N_new, D]) into the caches at positions [seqlens[b], seqlens[b] + N_new), in place; slots at or
    beyond the capacity are dropped (the GPU kernel's rule)."""
    page = k_cache.shape[2]
    capacity = page * block_table.shape[1] if block_table is not None else k_cache.shape[2]
    for b, start in enumerate(seqlens):
        for t in range(k_new.shape[2]):
            pos = start + t
            if pos >= capacity:
                break
            if block_table is None:
                k_cache[b, :, pos] = k_new[b, :, t]
                v_cache[b, :, pos] = v_new[b, :, t]
            else:
                blk = int(block_table[b, pos // page])
                k_cache[blk, :, pos % page] = k_new[b, :, t]
                v_cache[blk, :, pos % page] = v_new[b, :, t]


E4M3_MAX = 448.0


def quantise_e4m3(x, scale):
    """The append rule of an fp8 cache: e4m3_rne(clamp(float(x) / scale, -448, 448)) as float8_e4m3fn; scale broadcasts against x.  The
    divide is float32's correctly rounded one, finite values saturate at +-448 (the explicit clamp), NaN stays NaN."""
    return (x.float() / scale).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)


def attention_forward_kvcache_cpu(q, k_cache, v_cache, k_new, v_new, seqlens, block_table=None, scale=8.0, groups=1, causal=False,
                                  l2norm_qk=True, window_size=(-1, -1), k_scale=None, v_scale=None, return_lse=False, tree_words=None,
                                  alibi_slopes=None):
    """Forward-only path of `flash_cosine_sim_attention_with_kvcache` on host tensors: the append as an indexed copy, then the dense CPU
    forward of every sequence over its first L_b = seqlens[b] + N_new cached positions (o = 0 where L_b == 0).  seqlens: host ints.
    k_scale / v_scale (float32 [B, Hk], both or neither): the caches are float8_e4m3fn codes meaning scale * code -- the append quantises
    (quantise_e4m3), and each sequence's keys and values are dequantised to float32 for the dense forward, whose result is cast to q's
    dtype.  return_lse: also the rows' log-sum-exp, float32 [B, H, N] (-inf where a row sees no key; k_scale is inside the logits, v_scale
    is not).  tree_words: int64 [N] (batch 1, the varlen path below): the rows' visibility words over the last N positions (`tree_tail`) in
    place of causal.  alibi_slopes: float32 [H] or [B, H]: the linear position bias of `attention_forward_cpu`, per sequence."""
    fp8 = k_scale is not None
    if k_new is not None:
        if fp8:
            append_kvcache_cpu(k_cache.view(torch.uint8), v_cache.view(torch.uint8),
                               quantise_e4m3(k_new, k_scale[:, :, None, None]).view(torch.uint8),
                               quantise_e4m3(v_new, v_scale[:, :, None, None]).view(torch.uint8), seqlens, block_table)
        else:
            append_kvcache_cpu(k_cache, v_cache, k_new, v_new, seqlens, block_table)
    n_new = 0 if k_new is None else k_new.shape[2]
    out = torch.zeros_like(q)
    lse = torch.full(q.shape[:-1], float("-inf"), dtype=torch.float32)
    for b, start in enumerate(seqlens):
        length = start + n_new
        if length == 0 or q.shape[2] == 0:
            continue
        kb, vb = cache_gather(k_cache, b, length, block_table), cache_gather(v_cache, b, length, block_table)
        qb = q[b:b + 1]
        if fp8:
            qb = qb.float()
            kb, vb = kb.float() * k_scale[b][None, :, None, None], vb.float() * v_scale[b][None, :, None, None]
        tail = None if tree_words is None else tree_tail(tree_words, length)
        slopes = None if alibi_slopes is None else (alibi_slopes if alibi_slopes.dim() == 1 else alibi_slopes[b])
        out[b:b + 1], lse[b:b + 1] = attention_forward_cpu(qb, kb, vb, scale=scale, groups=groups, causal=causal, l2norm_qk=l2norm_qk,
                                                           window_size=window_size, return_lse=True, tail_mask=tail, alibi_slopes=slopes)
    return (out, lse) if return_lse else out


TREE_MAX_TOKENS = 64


def tree_tail(words, length):
    """The visibility words of a tree step's N <= 64 rows (int64 [N], read as unsigned: bit t of word i set = query i sees the step's token
    t, cache position length - N + t) as the bool matrix [N, T] over the last T = min(N, length) positions: positions below 0 do not exist."""
    n = words.numel()
    bits = ((words.reshape(n, 1) >> torch.arange(TREE_MAX_TOKENS, dtype=torch.int64)) & 1).bool()[:, :n]      # (>> is arithmetic: & 1 keeps the bit)
    return bits[:, n - min(n, length):]


def attention_forward_kvcache_varlen_cpu(q, k_cache, v_cache, cu_seqlens_q, k_new, v_new, seqlens, block_table=None, scale=8.0, groups=1,
                                         causal=False, l2norm_qk=True, window_size=(-1, -1), k_scale=None, v_scale=None,
                                         return_lse=False, tree_mask=None, alibi_slopes=None):
    """Forward-only path of `flash_cosine_sim_attention_varlen_with_kvcache` on host tensors: packed q [total_q, H, D] and k_new / v_new
    [total_q, Hk, D] with a validated host table; sequence b's N_b rows run through `attention_forward_kvcache_cpu` as a batch-1 call on
    its own cache (a view: the append lands in the caller's caches), so its rows and its cache slots are exactly what the equal-N path
    gives for that sequence alone.  seqlens: host ints, tokens cached before the append.  return_lse: also the rows' log-sum-exp, float32 [total_q, H].
    tree_mask (`flash_cosine_sim_attention_tree_with_kvcache`): int64 [total_q] packed like q (no causal, no window with it): with
    P_b = L_b - N_b every query of sequence b sees the cache positions before P_b, and query i sees position P_b + t iff bit t of its word is set; a sequence with N_b > 64 ignores its words and is
    causal.
    alibi_slopes (`flash_cosine_sim_attention_alibi_with_kvcache`): float32 [H] or [B, H]: the logit of key j for query i of sequence b gains
    -slope[b, h] * |L_b - N_b + i - j|.  It combines with causal and window_size, not with tree_mask."""
    if tree_mask is not None and (causal or tuple(window_index(window_size)) != (-1, -1)):
        raise ValueError("tree_mask states the visibility: no causal and no window_size with it")
    if tree_mask is not None and alibi_slopes is not None:
        raise ValueError("alibi_slopes is not taken with a tree_mask: a tree token's position is its depth, not its slot")
    out = torch.zeros_like(q)
    lse = torch.full(q.shape[:-1], float("-inf"), dtype=torch.float32)
    cq = cu_seqlens_q.tolist()
    for b in range(len(cq) - 1):
        lo, hi = cq[b], cq[b + 1]
        if hi == lo:
            continue
        rows = lambda t: None if t is None else t[lo:hi].permute(1, 0, 2).unsqueeze(0)      # [1, heads, N_b, D]
        paged = block_table is not None
        kc, vc = (k_cache, v_cache) if paged else (k_cache[b:b + 1], v_cache[b:b + 1])
        quant = {} if k_scale is None else dict(k_scale=k_scale[b:b + 1], v_scale=v_scale[b:b + 1])
        words = tree_mask[lo:hi] if tree_mask is not None and hi - lo <= TREE_MAX_TOKENS else None
        slopes = None if alibi_slopes is None else (alibi_slopes if alibi_slopes.dim() == 1 else alibi_slopes[b])      # [H] of this sequence
        o, l = attention_forward_kvcache_cpu(rows(q), kc, vc, rows(k_new), rows(v_new), [seqlens[b]], block_table[b:b + 1] if paged else None,
                                             scale=scale, groups=groups, causal=causal or (tree_mask is not None and words is None),
                                             l2norm_qk=l2norm_qk, window_size=window_size, return_lse=True, tree_words=words,
                                             alibi_slopes=slopes, **quant)
        out[lo:hi] = o[0].permute(1, 0, 2)
        lse[lo:hi] = l[0].permute(1, 0)
    return (out, lse) if return_lse else out


def merge_attention_states_cpu(os, lses):
    """`merge_attention_states` on host tensors, in float32: M = max_s lse_s; every state empty (M == -inf): o = 0, lse = -inf; else
    w_s = exp(lse_s - M), W = sum_s w_s, o = (sum_s w_s * o_s) / W rounded once, lse = M + log(W).  A state of weight 0 is skipped, as in
    the kernel: its o_s cannot leak (NaN included), and the first live product of a row is assigned rather than added to +0, so one state
    beside empty ones comes back bit for bit, -0 included.  Made of torch ops that autograd differentiates
    (`merge_attention_states_with_grad`): a skipped state's o_s is replaced by 0 BEFORE the product, so its NaNs reach neither the result
    nor a gradient."""
    lse = torch.stack([l.float() for l in lses])                       # [S, ...]
    top = lse.amax(dim=0)
    live = top > float("-inf")
    safe = torch.where(live, top, torch.zeros_like(top))
    w = torch.where(lse > float("-inf"), torch.exp(lse - safe), torch.zeros_like(lse))
    total = w.sum(dim=0)
    zero = torch.zeros((), dtype=torch.float32)
    acc = torch.zeros(os[0].shape, dtype=torch.float32)
    started = torch.zeros(top.shape, dtype=torch.bool).unsqueeze(-1)
    for s, o in enumerate(os):
        alive = (w[s] != 0).unsqueeze(-1)
        term = w[s].unsqueeze(-1) * torch.where(alive, o.float(), zero)
        acc = torch.where(alive, torch.where(started, acc + term, term), acc)
        started = started | alive
    total = torch.where(live, total, torch.ones_like(total))
    out = torch.where(live.unsqueeze(-1), acc / total.unsqueeze(-1), zero)
    out_lse = torch.where(live, safe + torch.log(total), torch.full_like(top, float("-inf")))
    return out.to(os[0].dtype).contiguous(), out_lse.contiguous()


def kvcache_keep_accepted_cpu(k_cache, v_cache, seqlens, accepted, num_accepted, block_table=None):
    """`kvcache_keep_accepted` on host tensors, in place: for i < num_accepted[b] the row at cache position seqlens[b] + accepted[b][i] moves
    to seqlens[b] + i, in K and in V, for every K/V head.  Every source row is read before the first is written (destination i of one move
    can be the source of another); a move whose source or destination is at or beyond the capacity is skipped.  seqlens, accepted and
    num_accepted: host lists (validated by the caller).  Rows move as they are, so fp8 caches go through their uint8 views."""
    page = k_cache.shape[2]
    capacity = page * block_table.shape[1] if block_table is not None else k_cache.shape[2]
    if k_cache.dtype == getattr(torch, "float8_e4m3fn", None):
        k_cache, v_cache = k_cache.view(torch.uint8), v_cache.view(torch.uint8)

    def row(cache, b, pos):
        if block_table is None:
            return cache[b, :, pos]
        return cache[int(block_table[b, pos // page]), :, pos % page]

    for b, start in enumerate(seqlens):
        moves = [(start + accepted[b][i], start + i) for i in range(num_accepted[b])]
        moves = [(src, dst) for src, dst in moves if src != dst and src < capacity and dst < capacity]
        held = [(row(k_cache, b, src).clone(), row(v_cache, b, src).clone()) for src, _ in moves]
        for (_, dst), (kr, vr) in zip(moves, held):
            row(k_cache, b, dst).copy_(kr)
            row(v_cache, b, dst).copy_(vr)
