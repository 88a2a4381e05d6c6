"""Problems of `flash_cosine_sim_attention_alibi` -- one table for the GPU oracle test (test_gpu_alibi_train.py) and for the CPU coverage
test that checks, with the alibi launch recorder, that the table launches every `*_alibi_kernel` instantiation a call can reach
(test_alibi_forms_cpu.py).  No torch here: plain tuples, as in window_cases.py, whose grids, dtype codes and keyword helpers are used.

Every call with slopes is a windowed launch (open sides where it has no window), so its form depends on what a windowed launch's form
depends on: dtype, D, batch x heads, N (forward, dQ) or M (dK/dV), the shift regime and the CU count.  A non-causal call needs N <= M.
"""
import window_cases as W

DTYPES, DIMS, DTYPE_CODE, GRIDS = W.DTYPES, W.DIMS, W.DTYPE_CODE, W.GRIDS

# windows of the cases, by turns: none, causal, the two of the issue, and two that put the left edge inside the first / a later tile
WINDOWS = ((-1, -1, False), (-1, -1, True), (64, 0, True), (129, 64, False), (31, 0, True), (200, -1, False))


def standard_slopes(H):
    """2^(-8 (h + 1) / H), the ALiBi paper's geometric sequence"""
    return [2.0 ** (-8.0 * (h + 1) / H) for h in range(H)]


def batch_slopes(B, H):
    """[B, H]: the standard slopes, scaled per batch entry / sequence so that no two rows are equal (and one row is all zero)"""
    return [[s * ((b * 3) % 4) / 2.0 for s in standard_slopes(H)] for b in range(B)]


def _edge_cases():
    """B 2, H 8: the lengths that cross the 128-row / 64-key tile boundaries, the bottom-right offset both ways (N < M; causal N > M, whose
    first rows see no key), D 64 / 128 in every dtype and D 16 / 96 in bf16, f16 at scale 16 (the per-row-shift forms), H 8 over Hk 2 / 8,
    [H] and [B, H] slopes, the windows above -- by turns, so that every value of each list meets several of the others"""
    shapes = ((127, 127, None), (128, 128, None), (129, 129, None), (257, 257, None), (100, 300, None), (300, 100, True))
    types = (("bf16", 64), ("f16", 64), ("f32", 64), ("bf16", 128), ("f16", 128), ("f32", 128), ("bf16", 16), ("bf16", 96))
    out, i = [], 0
    for N, M, force_causal in shapes:
        for dtype, D in types:
            left, right, causal = WINDOWS[i % len(WINDOWS)]
            if force_causal:
                left, right, causal = (WINDOWS[1], WINDOWS[2], WINDOWS[4])[i % 3]
            Hk = (2, 8)[(i // 2) % 2]
            kind = ("h", "bh")[(i // 3) % 2]
            kw = dict(causal=causal)
            if dtype == "f16" and i % 2 == 1:
                kw.update(scale=16.0)
            elif i % 5 == 4:
                kw.update(groups=2, scale=4.0)
            out.append((f"edge_{dtype}_d{D}_n{N}m{M}_w{left}_{right}_{'causal' if causal else 'full'}_k{Hk}_{kind}_{i}",
                        dtype, D, 2, 8, Hk, N, M, left, right, kw, kind))
            i += 1
    # f16 at scale 16 on every boundary length, D 64 and 128 (the per-row-shift forms see the biased logits in their online maximum)
    for j, (N, M) in enumerate(((127, 127), (129, 129), (257, 257), (100, 300))):
        for D in (64, 128):
            left, right, causal = WINDOWS[(j + D // 64) % 4]
            out.append((f"edge_f16_d{D}_n{N}m{M}_scale16_w{left}_{right}_{'causal' if causal else 'full'}", "f16", D, 2, 8, (2, 8)[j % 2], N, M, left,
                        right, dict(causal=causal, scale=16.0), ("h", "bh")[j % 2]))
    return out


def _form_candidates():
    """the grids of window_cases.GRIDS x dtype x head dim x shift regime, as window_cases._form_cases builds them, with N <= M where the
    call is not causal"""
    out, i = [], 0
    for dtype in DTYPES:
        for D in DIMS:
            for grid in GRIDS:
                for per_row in (False, True):
                    B, H, L = GRIDS[grid]
                    Hk = (H, H // 2, 1)[i % 3]
                    left, right, causal = WINDOWS[i % len(WINDOWS)]
                    kw = dict(W.per_row_kwargs(dtype, i) if per_row else W.static_kwargs(D, i), causal=causal)
                    N, M = (L, L) if i % 4 < 2 else (L - 43, L) if (i % 4 == 2 or not causal) else (L, L - 40)
                    name = f"{dtype}_d{D}_{grid}_{'per_row' if per_row else 'static'}_w{left}_{right}_{'causal' if causal else 'full'}_h{H}k{Hk}_n{N}m{M}"
                    out.append((name, dtype, D, B, H, Hk, N, M, left, right, kw, ("h", "bh")[i % 2]))
                    i += 1
    return out


FORM_CANDIDATES = _form_candidates()
# The candidates the GPU test runs: a subset that still launches every reachable instantiation (chosen greedily with the recorder;
# test_alibi_forms_cpu.py fails when it stops covering).  None: all of them.
FORM_PICK = (0, 1, 2, 3, 7, 8, 9, 10, 11, 14, 15, 16, 17, 18, 19, 23, 24, 25, 31, 32, 33, 39, 40, 41, 42, 43, 46, 47, 48, 49, 50, 51, 54, 55, 56, 57,
             58, 59, 62, 64, 67, 70, 71, 72, 73, 80, 81, 84, 85, 88, 89, 92, 93, 97, 104, 105, 113)
FORM_CASES = FORM_CANDIDATES if FORM_PICK is None else [FORM_CANDIDATES[i] for i in FORM_PICK]
EDGE_CASES = _edge_cases()
# id, dtype, D, B, H, Hk, N, M, left, right, kwargs, slopes kind ("h": [H], "bh": [B, H])
DENSE_CASES = EDGE_CASES + FORM_CASES

# packed, causal: id, dtype, D, H, Hk, left, right, kwargs, slopes kind; the lengths of every case: PACKED_LENGTHS (an empty sequence last)
PACKED_LENGTHS = (1, 130, 257, 64, 0)
PACKED_CASES = [
    ("packed_bf16_d64_k2_h", "bf16", 64, 8, 2, -1, -1, dict(causal=True), "h"),
    ("packed_f16_d128_k8_bh_w64", "f16", 128, 8, 8, 64, 0, dict(causal=True), "bh"),
    ("packed_f32_d64_k2_bh", "f32", 64, 8, 2, -1, -1, dict(causal=True), "bh"),
    ("packed_f16_d64_scale16_k8_h", "f16", 64, 8, 8, -1, -1, dict(causal=True, scale=16.0), "h"),
    ("packed_bf16_d96_k2_h_w31", "bf16", 96, 8, 2, 31, 0, dict(causal=True), "h"),
]


def recorder_line(dtype, D, B, H, Hk, N, M, left, right, kw, kind=None, cus=256, tail=""):
    """the alibi recorder's input line of a dense problem (tests/native/alibi_launch_recorder.cpp)"""
    return W.recorder_line(dtype, D, B, H, Hk, N, M, left, right, kw, cus=cus, tail=tail)
