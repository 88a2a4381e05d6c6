"""Masks, visibility matrices and batches of the tree-attention tests (test_kvcache_tree_cpu.py, test_gpu_kvcache_tree.py).  No GPU code.

A tree step's rule, from the docstring of flash_cosine_sim_attention_tree_with_kvcache: with L the sequence's length after the step and
P = L - N, every query sees the cache positions j < P; query i sees position P + t (the step's token t, 0 <= t < N) iff bit t of its 64-bit
word is set; positions below 0 (N > L) do not exist; a sequence with N > 64 ignores its words and is causal, bottom-right aligned."""
import numpy as np
import torch

MAX_TOKENS = 64

# row tile of exactly 16 rows at Hk == H; the batch of the decidability condition and the probe ...
N_B = [1, 0, 5, 16, 37, 64, 7, 33]
CACHED = [0, 17, 300, 5, 0, 1023, 40, 95]
CAPACITY = 1200
# ... and the same counts in a cache short enough for one key split on both sides of an identity
BIT_CACHED = [0, 17, 150, 5, 0, 170, 40, 95]
BIT_CAP = 240
# the probed (dtype, D) pairs
PROBE_TYPES = (("bf16", 64), ("f16", 128), ("f32", 32), ("f16", 16))


def chain(n):
    """word i = bits 0 .. i: what causal=True sees"""
    return [(1 << (i + 1)) - 1 for i in range(n)]


def full(n):
    """every bit set (the bits at and beyond n are never looked at): what causal=False sees"""
    return [(1 << MAX_TOKENS) - 1] * n


def random_tree(n, rng):
    """token 0 is the root, the parent of token t is uniform in [0, t); word = ancestors and self"""
    words = []
    for t in range(n):
        words.append((1 << t) | (words[int(rng.integers(0, t))] if t else 0))
    return words


def random_bits(n, rng):
    """any 64-bit word per row: no tree, no diagonal, garbage in the bits at and beyond n; every fifth row sees none of the step's tokens"""
    return [0 if i % 5 == 4 else int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)) for i in range(n)]


KINDS = {"chain": lambda n, rng: chain(n), "full": lambda n, rng: full(n), "tree": random_tree, "bits": random_bits}


def words_of(kind, counts, seed=0):
    """the unsigned words of a packed batch, sequence by sequence"""
    rng = np.random.default_rng(seed)
    return [w & ((1 << MAX_TOKENS) - 1) for n in counts for w in KINDS[kind](n, rng)]      # (a sequence of more than 64 tokens ignores its words)


def as_int64(words, device="cpu"):
    """unsigned 64-bit words as the int64 tensor the call takes (bit 63 is the sign)"""
    return torch.tensor([w - (1 << 64) if w >= 1 << 63 else w for w in words], dtype=torch.int64, device=device)


def visibility(words, n, length):
    """bool [n, length] of ONE sequence: its n words against `length` cache positions, the step's tokens the last n of them"""
    j = np.arange(length)[None, :]
    p = length - n
    if n > MAX_TOKENS:
        return j <= np.arange(n)[:, None] + p
    vis = np.broadcast_to(j < p, (n, length)).copy()
    for i, w in enumerate(words):
        for t in range(max(-p, 0), n):
            vis[i, p + t] = bool((w >> t) & 1)
    return vis


def split_words(words, counts):
    out, at = [], 0
    for n in counts:
        out.append(words[at:at + n])
        at += n
    return out


def bias_of(vis):
    """0 where visible, -inf where not: the additive bias of the float64 oracle, [1, n, length]"""
    return np.where(vis, 0.0, -np.inf)[None]


def cu_of(counts, device="cpu"):
    return torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=device)


def run_probe(dtype, D, H, Hk, kind, device, page=0, fp8=False, scale=8.0, seed=0, flip=None, operand_dtype=None):
    """flash_cosine_sim_attention_tree_with_kvcache with tree_mask and return_lse on the cone inputs of visibility_probe.py (its
    run_decode with a mask in place of causal): the batch N_B against CACHED, every query bringing its key.  Returns the comparisons for
    visibility_probe.judge and the visibility matrix of every sequence.  flip = (packed row, bit): that bit of the mask HANDED TO THE CALL
    is inverted while the expectation keeps the original -- a single hidden or leaked key, which the judge must catch.  operand_dtype: the
    type the logit's operands are rounded to (default: q's; the CPU path normalises an fp8 cache's keys in float32)."""
    import visibility_probe as VP
    F = VP._F()
    B = len(N_B)
    scales = (0.5, 2.0) if fp8 else None
    kc, vc, table = VP._cache(dtype, D, B, Hk, CAPACITY, page, CACHED, True, seed + 7, scales)
    words = words_of(kind, N_B, seed)
    qs, kns, vns, refs_o, refs_l, views = [], [], [], [], [], []
    for b, (n, own) in enumerate(zip(N_B, split_words(words, N_B))):
        q, _, _ = VP.probe_queries(dtype, (H,), n, D, True, seed + 3 * b)
        kn, vn, _ = VP.probe_keys(dtype, (Hk,), n, D, True, seed + 3 * b + 1, pos=torch.arange(n) + CACHED[b])
        qs.append(q), kns.append(kn), vns.append(vn)
        views.append(visibility(own, n, CACHED[b] + n))
        e = VP.expected(views[-1], D, operand_dtype or dtype, scale, True, grads=False)
        refs_o.append(e["o"]), refs_l.append(e["lse"])
    given = list(words)
    if flip is not None:
        given[flip[0]] ^= 1 << flip[1]
    kw = dict(cache_seqlens=torch.tensor(CACHED, dtype=torch.int32), block_table=table, scale=scale, return_lse=True,
              tree_mask=as_int64(given, device))
    if fp8:
        kw.update(k_scale=scales[0], v_scale=scales[1])
    q = torch.cat([t.transpose(0, 1) for t in qs], 0).contiguous().to(device)
    kn, vn = (torch.cat([t.transpose(0, 1) for t in x], 0).contiguous().to(device) for x in (kns, vns))
    with torch.no_grad():
        o, lse = F.flash_cosine_sim_attention_tree_with_kvcache(q, kc.to(device), vc.to(device), cu_of(N_B), kn, vn, **kw)
    ref_o, ref_l = np.concatenate(refs_o, 0)[:, None, :], np.concatenate(refs_l, 0)[:, None]
    return [("o", "tree", o, ref_o, ref_o), ("lse", "tree", lse, ref_l, None)], views
