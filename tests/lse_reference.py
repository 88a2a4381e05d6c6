"""float64 references of the attention-state tests (test_kvcache_lse_cpu.py, test_gpu_kvcache_lse.py, test_gpu_shared_prefix.py): the
log-sum-exp of decoded rows, and the merge of attention states.  Built on the oracle's l2norm and operand rounding, so "operand-faithful"
means here what it means in the parity tests."""
import numpy as np

from oracle import cosine_sim_oracle as O

ULP = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 2.0 ** -24}


def derived_lse_bound(dtype, scale, groups, l2norm=True):
    """|dlse| against float64 on the RAW inputs: each logit moves by at most 2 u |scale| groups when c1 q^ and k^ are rounded to the type
    (u: the type's unit roundoff), an LSE by at most its logits' largest move; 1e-4 for float32 accumulation and the exponential.  Without
    l2norm_qk the 16-bit inputs are the operands themselves, so only the 1e-4 is left."""
    return (2 * ULP[dtype] * abs(scale) * groups if l2norm else 0.0) + 1e-4


def lse_rows(q, k, scale=8.0, groups=1, causal=False, l2norm_qk=True, operand_dtype=None, window=(-1, -1)):
    """Natural-log LSE of every row of ONE sequence: q [H, N, D], k [Hk, L, D] (float64; Hk divides H), the N queries being the last N of
    the L positions (bottom-right alignment).  window = (left, right), -1 unbounded, causal caps right at 0.  -inf where no key is visible."""
    q, k = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64)
    H, N, _ = q.shape
    Hk, L, _ = k.shape
    if l2norm_qk:
        q, k = O.l2norm(q, groups), O.l2norm(k, groups)
        q, k = O.rounded_operands(q, k, scale, operand_dtype)
    k = np.repeat(k, H // Hk, axis=0)
    s = np.einsum("hid,hjd->hij", q, k) * scale
    i = np.arange(N)[:, None] + (L - N)
    j = np.arange(L)[None, :]
    left, right = window
    right = 0 if causal else right
    vis = np.ones((N, L), dtype=bool)
    if right >= 0:
        vis &= j <= i + right
    if left >= 0:
        vis &= j >= i - left
    s = np.where(vis[None], s, -np.inf)
    top = s.max(axis=-1, initial=-np.inf)
    safe = np.where(np.isfinite(top), top, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(top), safe + np.log(np.exp(s - safe[..., None]).sum(-1)), -np.inf)


def merge_reference(os, lses):
    """The merge of attention states in float64 on the (o_s, lse_s) given: (o, lse); a state with lse = -inf contributes nothing whatever
    its o holds."""
    lse = np.stack([np.asarray(l, dtype=np.float64) for l in lses])
    top = lse.max(axis=0)
    live = np.isfinite(top)
    safe = np.where(live, top, 0.0)
    w = np.where(np.isfinite(lse), np.exp(lse - safe), 0.0)
    total = w.sum(0)
    acc = 0.0
    for s, o in enumerate(os):
        acc = acc + np.where((w[s] != 0)[..., None], w[s][..., None] * np.nan_to_num(np.asarray(o, dtype=np.float64)), 0.0)
    total1 = np.where(live, total, 1.0)
    return np.where(live[..., None], acc / total1[..., None], 0.0), np.where(live, safe + np.log(total1), -np.inf)
