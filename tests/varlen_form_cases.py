"""Ragged packed-sequence problems on every kernel form the dispatch gives packed sequences -- one table for the GPU oracle test
(test_gpu_varlen.py::test_varlen_forms) and the CPU coverage test that checks, with the launch recorder, that the table launches every
attention-kernel instantiation a varlen call can reach (test_varlen_forms_cpu.py); the same for the 8-wave bit-for-bit and buffer-bounds
shapes at the end.  No torch here: plain tuples.

A varlen launch's form depends only on sequences x heads, max_seqlen and the CU count (256 on MI355X); the rows of each sequence only
decide what its workgroups do.  So every case packs the same ragged core of sequences -- empty query span, empty key span, one-row spans,
spans of t - 1, t, t + 1 for both tile sizes (128 and 256 positions), a span of three 256-position tiles, N_s != M_s both ways -- padded
with short sequences to the sequence count its grid needs, and reaches chip-filling grids with sequences and an inflated max_seqlen
rather than with rows: each case's float64 oracle stays near 1e8 multiply-adds.

The grids (w256 / w128: workgroups of 256- / 128-position tiles, causal: pairs of tiles; see tile_waves / choose_* in fcsa_dispatch.h):
    "full"   w256 in [224, 256]             8-wave forms: forward Rows8 / Lean8, dQ Waves8 / Waves4Two, dK/dV Waves8 / Lean8
    "tail"   w256 > 256, last round <= 55 %  16-bit rows <= 128 bytes: the 4-wave forms everywhere (the last-round rule)
    "small"  w128 <= 256, w256 < 224         key-split forward and dQ, query-split dK/dV (>= 512 queries), 4-wave forms otherwise
"""

DTYPES = ("bf16", "f16", "f32")
DIMS = (16, 32, 64, 96, 128)
CORE_Q = [0, 1, 7, 127, 128, 129, 255, 256, 257, 600, 40]
CORE_K = [5, 9, 0, 129, 128, 127, 257, 256, 255, 560, 1]

# grid -> causal -> inflated max_seqlen (None: exact, the longest span) -> sequences x heads
GRIDS = {
    "full": {0: {2048: 32, None: 80}, 1: {2048: 64, None: 120}},
    "tail": {0: {2048: 38, None: 100}, 1: {2048: 76, None: 150}},
    "small": {0: {2048: 12, None: 48}, 1: {2048: 24, None: 48}},
}


def _grids(dtype, D):
    """the grids whose forms differ for this dtype and head dim"""
    if dtype == "f32":
        return ("full", "small") if D <= 32 else ("small",)
    return ("full", "tail", "small") if D <= 64 else ("full", "small")


def _heads(sh, D):
    """the most heads (8, 4, 2, 1) dividing sequences x heads with at least a dozen sequences and H x D <= 256"""
    return next(h for h in (8, 4, 2, 1) if sh % h == 0 and sh // h >= 12 and h * D <= 256)


def _kwargs(dtype, D, per_row, i):
    """static exponent shift: fused q-l2norm (groups = 1), the row-kernel l2norm (groups of 4 features: never fusable), or inputs already
    unit-norm (l2norm_qk=False); per-row shift: scale x groups beyond the static window (f16: > 11, bf16 / f32: > 75)"""
    if per_row:
        top = 16.0 if dtype == "f16" else 80.0
        return dict(scale=top) if (i // 4) % 2 == 0 else dict(groups=2, scale=top / 2)
    mode = i % 3
    if mode == 0:
        return dict()
    if mode == 1:
        return dict(groups=D // 4, scale=8.0 / (D // 4))
    return dict(l2norm_qk=False, scale=1.0)


def _cases():
    out, i = [], 0
    for dtype in DTYPES:
        for D in DIMS:
            for grid in _grids(dtype, D):
                for causal in (0, 1):
                    for per_row in (False, True):
                        inflated = (i // 2) % 2 == 0
                        mx = 2048 if inflated else None
                        sh = GRIDS[grid][causal][mx]
                        H = _heads(sh, D)
                        S = sh // H
                        Hk = (H, H // 2, 1)[(i + i // 3) % 3] if H >= 4 else (H, 1)[(i + i // 3) % 2]
                        pad = S - len(CORE_Q)
                        lq = CORE_Q + [(7 * j) % 23 for j in range(pad)]
                        lk = CORE_K + [(5 * j + 3) % 19 for j in range(pad)]
                        kw = dict(_kwargs(dtype, D, per_row, i), causal=bool(causal))
                        norm = "nol2" if not kw.get("l2norm_qk", True) else f"g{kw.get('groups', 1)}s{kw.get('scale', 8.0):g}"
                        name = f"{dtype}_d{D}_{grid}_{'causal' if causal else 'full'}_{'per_row' if per_row else 'static'}_{norm}_h{H}k{Hk}" + \
                               ("_maxlen2048" if inflated else "")
                        out.append((name, dtype, D, lq, lk, H, Hk, mx, kw))
                        i += 1
    return out


# id, dtype, D, query lengths, key lengths, H, Hk, max_seqlen (q and k; None: the longest spans), kwargs
CASES = _cases()

# Equal-length sequences on which the packed call and the dense [S, H, L, D] call launch the same 8-wave instantiation (forward Rows8 /
# Lean8, dQ Waves8 / Waves4Two, dK/dV Waves8 / Lean8) with the same grid -- with the dense 64-rows-per-wave D = 128 forward turned off
# (fcsa_debug_forward_form(0)); D = 32 stays below the dense fwd2 threshold (4096 keys).  Must match bit for bit
# (test_gpu_varlen.py::test_varlen_equal_lengths_match_dense_bit_for_bit; the recorder confirms the launches in test_varlen_forms_cpu.py).
# id, dtype, S, H, L, D, causal
BIT_CASES = [
    ("bf16_d64_rows8", "bf16", 4, 8, 2048, 64, False),
    ("f16_d64_causal_rows8", "f16", 8, 8, 2048, 64, True),
    ("bf16_d32_rows8", "bf16", 4, 8, 2048, 32, False),
    ("f32_d32_causal_rows8", "f32", 8, 8, 2048, 32, True),
    ("bf16_d128_causal_lean8", "bf16", 8, 8, 2048, 128, True),
    ("f16_d96_lean8", "f16", 4, 8, 2048, 96, False),
    ("f16_d128_lean8", "f16", 4, 8, 2048, 128, False),
]

# Caller-owned buffers in a NaN-filled arena (test_gpu_varlen.py::test_varlen_calls_stay_inside_their_buffers) on grids that take the
# 8-wave forms: 28 sequences x 8 heads of at most 256 rows (224 workgroups of 256-position tiles), or 14 x 8 of up to 384 (dQ: the
# two-wave tile).  The last sequence ends inside a tile, flush against the guard band behind k / v: an unmasked read past total_k
# would bring NaN into the outputs.
# id, dtype, query lengths, key lengths, H, Hk, D, kwargs
BOUNDS_CASES = [
    ("bf16_d64_rows8", "bf16",
     [8, 61, 114, 0, 220, 17, 70, 123, 176, 229, 26, 79, 132, 185, 238, 35, 88, 141, 194, 247, 44, 97, 150, 203, 256, 53, 106, 201],
     [12, 49, 86, 123, 160, 0, 234, 15, 52, 89, 126, 163, 200, 237, 18, 55, 92, 129, 166, 203, 240, 21, 58, 95, 132, 169, 206, 131],
     8, 8, 64, dict()),
    ("f16_d64_causal_rows8_gqa", "f16",
     [4, 45, 86, 127, 168, 209, 0, 35, 76, 117, 158, 199, 240, 25, 66, 107, 148, 189, 230, 15, 56, 97, 138, 179, 220, 5, 46, 199],
     [18, 47, 0, 105, 134, 163, 192, 221, 250, 23, 52, 81, 110, 139, 168, 197, 226, 255, 28, 57, 86, 115, 144, 173, 202, 231, 4, 250],
     8, 2, 64, dict(causal=True)),
    ("bf16_d128_causal_lean8", "bf16",
     [6, 53, 100, 147, 0, 241, 32, 79, 126, 173, 220, 11, 58, 105, 152, 199, 246, 37, 84, 131, 178, 225, 16, 63, 110, 157, 204, 255],
     [14, 45, 76, 107, 138, 169, 200, 0, 6, 37, 68, 99, 130, 161, 192, 223, 254, 29, 60, 91, 122, 153, 184, 215, 246, 21, 52, 129],
     8, 8, 128, dict(causal=True)),
    ("f16_d128_lean8_two_wave_dq", "f16",
     [384, 77, 0, 211, 278, 345, 28, 95, 162, 229, 296, 363, 46, 300],
     [20, 63, 106, 149, 192, 235, 278, 321, 364, 0, 66, 109, 152, 257],
     8, 8, 128, dict()),
]
