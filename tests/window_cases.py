"""Sliding-window problems -- one table for the GPU oracle tests (test_gpu_window.py) and for the CPU coverage test that checks, with the
window launch recorder, that the table launches every windowed kernel instantiation a call can reach (test_window_forms_cpu.py).  No
torch here: plain tuples.

A windowed launch is dispatched like a packed one (choose_* with varlen = true, fcsa_dispatch.h) and always as a causal grid (pairs of
tiles), so its form depends only on dtype, D, batch x heads, N (forward, dQ) or M (dK/dV), the shift regime and the CU count (256 on
MI355X).  Chip-filling grids are reached with heads, not rows: the float64 oracle of a case runs on two (batch, K/V head) slices, and the
whole output is compared with the existing attn_bias route on the 0 / -inf band.

The grids (w256 / w128: workgroups of 256- / 128-row tiles, in causal pairs; tile_waves / choose_*):
    "full"   w256 in [224, 256]              8-wave forms: forward Rows8 / Lean8, dQ Waves8 / Waves4Two, dK/dV Waves8 / Lean8
    "tail"   w256 > 256, last round <= 55 %   16-bit rows <= 128 bytes: the 4-wave forms (the last-round rule)
    "mid"    w128 > 256 > w256, w256 < 224    16-bit: the 8-wave forms from 132 workgroups on; float32: 4 waves
    "small"  w128 <= 256                      key-split forward and dQ, query-split dK/dV (>= 512 queries), 4-wave forms otherwise
"""

DTYPES = ("bf16", "f16", "f32")
DIMS = (16, 32, 64, 96, 128)
DTYPE_CODE = {"f32": 0, "f16": 1, "bf16": 2}

# grid -> (batch, heads, N = M)
GRIDS = {"full": (8, 30, 300), "tail": (10, 30, 300), "mid": (5, 30, 300), "small": (1, 8, 1100)}
# windows of the form cases, by turns: narrower than a tile, about a tile, wider than three 64-key tiles, with a right side
FORM_WINDOWS = ((31, 0, True), (64, 0, True), (200, 0, True), (129, 64, False), (1, 0, True), (300, 1, False), (63, -1, False), (128, 200, False))


def per_row_kwargs(dtype, i):
    """scale x groups beyond the static exponent window (f16: > 11, bf16 / f32: > 75)"""
    top = 16.0 if dtype == "f16" else 80.0
    return dict(scale=top) if i % 2 == 0 else dict(groups=2, scale=top / 2)


def static_kwargs(D, i):
    """fused q-l2norm (groups = 1), the row-kernel l2norm (groups of 4 features: never fusable), inputs already unit-norm"""
    return (dict(), dict(groups=D // 4, scale=8.0 / (D // 4)), dict(l2norm_qk=False, scale=1.0))[i % 3]


def _form_cases():
    out, i = [], 0
    for dtype in DTYPES:
        for D in DIMS:
            for grid in GRIDS:
                for per_row in (False, True):
                    B, H, L = GRIDS[grid]
                    Hk = (H, H // 2, 1)[i % 3]
                    left, right, causal = FORM_WINDOWS[i % len(FORM_WINDOWS)]
                    kw = dict(per_row_kwargs(dtype, i) if per_row else static_kwargs(D, i), causal=causal)
                    # N != M by turns (the grid class is decided by N for forward / dQ and M for dK/dV: keep both in the same class)
                    N, M = (L, L) if i % 4 < 2 else (L, L - 40) if i % 4 == 2 else (L - 43, L)
                    name = f"{dtype}_d{D}_{grid}_{'per_row' if per_row else 'static'}_w{left}_{right}_{'causal' if causal else 'full'}_h{H}k{Hk}_n{N}m{M}"
                    out.append((name, dtype, D, B, H, Hk, N, M, left, right, kw))
                    i += 1
    return out


# id, dtype, D, B, H, Hk, N, M, left, right, kwargs
FORM_CASES = _form_cases()

LEFTS = (0, 1, 31, 32, 63, 64, 127, 128, 129, 300, 5000)
RIGHTS = (-1, 0, 1, 64, 200)
LENGTHS = (127, 128, 129, 255, 256, 257)


def _edge_cases():
    """small grids: every left x right of the lists above on N = M, N < M and N > M (rows without a visible key) with lengths of t - 1, t,
    t + 1 for t = 128 and 256, dtypes / head dims / K/V groupings / shift regimes by turns"""
    out, i = [], 0
    for left in LEFTS:
        for right in RIGHTS:
            dtype, D = DTYPES[i % 3], DIMS[(i // 3) % 5]
            causal = i % 2 == 1
            L = LENGTHS[i % len(LENGTHS)]
            # (i = 5 x the index of left + the index of right: the shape goes with their sum, so every right meets every N / M relation)
            N, M = ((L, L), (L, L + 150), (L + 150, L), (50, 20), (L, 2 * L + 1))[(i // 5 + i) % 5]
            H = 4
            Hk = (4, 2, 1)[(i // 2) % 3]
            if i % 7 == 3:
                kw = per_row_kwargs(dtype, i)
            elif i % 7 == 5:
                kw = dict(l2norm_qk=False, scale=1.0)
            elif i % 7 == 6:
                kw = dict(groups=2, scale=4.0)
            else:
                kw = dict()
            kw = dict(kw, causal=causal)
            out.append((f"edge_{dtype}_d{D}_n{N}m{M}_w{left}_{right}_{'causal' if causal else 'full'}_k{Hk}_{i}", dtype, D, 1, H, Hk, N, M, left, right, kw))
            i += 1
    return out


EDGE_CASES = _edge_cases()
DENSE_CASES = EDGE_CASES + FORM_CASES

# packed: the ragged core of varlen_form_cases.CASES (empty spans included) under a window, small and chip-filling grids
# id, dtype, D, H, Hk, left, right, kwargs, padded sequence count (None: the core alone), max_seqlen (None: exact)
PACKED_CASES = [
    ("packed_bf16_d64_w100_causal", "bf16", 64, 4, 4, 100, 0, dict(causal=True), None, None),
    ("packed_f16_d128_w64_1", "f16", 128, 4, 2, 64, 1, dict(), None, None),
    ("packed_f32_d32_w31_causal", "f32", 32, 2, 1, 31, 0, dict(causal=True), None, None),
    ("packed_bf16_d96_w129_right_open", "bf16", 96, 2, 2, 129, -1, dict(), None, None),
    ("packed_f16_d64_per_row_w63", "f16", 64, 4, 4, 63, 0, dict(causal=True, scale=16.0), None, None),
    ("packed_bf16_d64_full_grid_w200", "bf16", 64, 8, 8, 200, 0, dict(causal=True), 15, 2048),
    ("packed_f16_d128_full_grid_w128_64", "f16", 128, 2, 2, 128, 64, dict(), 60, None),
    ("packed_bf16_d16_nol2_w1", "bf16", 16, 4, 2, 1, 0, dict(causal=True, l2norm_qk=False, scale=1.0), None, None),
]

# decode: id, dtype, D, B, H, Hk, N, capacity, page (0: contiguous), cache_seqlens before the append, appended keys, left, right, kwargs
DECODE_CASES = [
    ("decode_bf16_d128_n1_w300", "bf16", 128, 4, 8, 2, 1, 1024, 0, [1000, 37, 299, 640], 0, 300, -1, dict(causal=True)),
    ("decode_f16_d64_n5_w129_append", "f16", 64, 3, 4, 4, 5, 700, 0, [600, 3, 129], 5, 129, 0, dict(causal=True)),
    ("decode_bf16_d64_n1_paged_w64", "bf16", 64, 4, 8, 1, 1, 1024, 64, [900, 10, 64, 65], 1, 64, -1, dict()),
    ("decode_f32_d32_n5_paged_w31_2", "f32", 32, 2, 2, 2, 5, 512, 32, [500, 20], 5, 31, 2, dict()),
    ("decode_f16_d96_n5_w0", "f16", 96, 2, 4, 2, 5, 300, 0, [290, 1], 5, 0, 0, dict(causal=True)),
    ("decode_bf16_d16_n1_per_row_w200", "bf16", 16, 3, 2, 2, 1, 800, 0, [799, 150, 0], 1, 200, -1, dict(scale=80.0)),
    ("decode_bf16_d128_n1_long_w1024", "bf16", 128, 2, 8, 2, 1, 8192, 0, [8000, 500], 1, 1024, 0, dict(causal=True)),
]


def _decode_grid():
    """every decode_win instantiation: dtype x head dim x shift regime, and at D = 96 the l2norm group widths that straddle a lane's fragment
    (decode_groups_fast false: groups = 2, 48 features) in both regimes; N in {1, 5}, contiguous / paged, with / without an append by turns,
    ragged cache_seqlens shorter and longer than the window"""
    out, i = [], 0
    for dtype in DTYPES:
        for D in DIMS:
            for general in ((False, True) if D == 96 else (False,)):
                for per_row in (False, True):
                    top = 16.0 if dtype == "f16" else 80.0
                    if general:
                        kw = dict(groups=2, scale=top / 2 if per_row else 4.0)
                    else:
                        kw = per_row_kwargs(dtype, 0) if per_row else static_kwargs(D, 2 * i)      # (fused l2norm or unit-norm inputs)
                    N, page, n_new = (1, 5)[i % 2], (0, 32)[(i // 2) % 2], (0, 1, 5)[i % 3]
                    left, right, causal = ((70, 0, True), (33, -1, False), (129, 2, False), (0, 0, True))[i % 4]
                    H, Hk = ((4, 4), (8, 2), (4, 1))[i % 3]
                    name = f"decode_{dtype}_d{D}_{'general' if general else 'fast'}_{'per_row' if per_row else 'static'}_n{N}_p{page}_a{n_new}_w{left}_{right}"
                    out.append((name, dtype, D, 3, H, Hk, N, 512, page, [500, 40, 7], n_new, left, right, dict(kw, causal=causal)))
                    i += 1
    return out


DECODE_CASES += _decode_grid()


def decode_recorder_line(dtype, D, B, H, Hk, N, cap, page, lens, n_new, left, right, kw):
    """the window recorder's input line of a decode case: max_seqlen_k = the capacity, as the Python function passes it"""
    return recorder_line(dtype, D, B, H, Hk, N, cap, left, right, kw, tail=f" decode {cap} {page} {n_new}")


def recorder_line(dtype, D, B, H, Hk, N, M, left, right, kw, cus=256, tail=""):
    """the window recorder's input line of a dense problem (tests/native/window_launch_recorder.cpp)"""
    return (f"{cus} {DTYPE_CODE[dtype]} {D} {B} {H} {Hk} {N} {M} {int(kw.get('causal', False))} {int(kw.get('l2norm_qk', True))} "
            f"{kw.get('groups', 1)} {kw.get('scale', 8.0):g} {left} {right}{tail}\n")
