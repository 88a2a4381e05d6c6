"""Windowed, packed and decode problems at the sizes the README and profiles/window_ab.txt, varlen_ab.txt, decode_ab.txt quote speed for --
one table for the GPU tests (test_gpu_fullsize_features.py: float64 slices, exact probes, the bias route, identities) and for the CPU test
that pins what each case launches (test_fullsize_feature_launches_cpu.py, tests/golden/fullsize_feature_launches.txt).  No torch here.

The short tables (window_cases.py, varlen_form_cases.py, test_gpu_kvcache.py) reach chip-filling grids with heads and many short
sequences; the float64 numpy oracle keeps their spans at a few hundred rows.  Here a band is dozens of full tiles between two edge tiles,
a packed document runs for many tile rounds, and a decode call takes tens of key splits over a 32k cache.
"""
from window_cases import recorder_line

# ---- window, dense call: id, dtype, D, B, H, Hk, N, M, left, right, kwargs --------------------------------------------------------------
# bf16 (4, 8, N, D) causal, N in {4096, 8192, 16384} x left in {256, 1024, 4096} x D in {64, 128} thinned by turns: every N, every left,
# both D, and the half-length window N = 8192 / left = 4096 at D = 128 (left = 4096 at N = 4096 hides nothing: that is the causal call)
WINDOW_CASES = [
    ("win_bf16_n4096_l256_d64", "bf16", 64, 4, 8, 8, 4096, 4096, 256, 0, dict(causal=True)),
    ("win_bf16_n4096_l1024_d128", "bf16", 128, 4, 8, 8, 4096, 4096, 1024, 0, dict(causal=True)),
    ("win_bf16_n8192_l1024_d64", "bf16", 64, 4, 8, 8, 8192, 8192, 1024, 0, dict(causal=True)),
    ("win_bf16_n8192_l4096_d128", "bf16", 128, 4, 8, 8, 8192, 8192, 4096, 0, dict(causal=True)),
    ("win_bf16_n16384_l256_d128", "bf16", 128, 4, 8, 8, 16384, 16384, 256, 0, dict(causal=True)),
    ("win_bf16_n16384_l4096_d64", "bf16", 64, 4, 8, 8, 16384, 16384, 4096, 0, dict(causal=True)),
    # two-sided, N != M both ways (N > M: the first rows see no key)
    ("win_f16_two_sided_n4096_m6000_d64", "f16", 64, 2, 16, 16, 4096, 6000, 1000, 300, dict()),
    ("win_f16_two_sided_n6000_m4096_d128", "f16", 128, 2, 16, 16, 6000, 4096, 1000, 300, dict()),
    ("win_bf16_gqa_h32k8_n4096_d64", "bf16", 64, 4, 32, 8, 4096, 4096, 1024, 0, dict(causal=True)),
    # the per-row-shift regime, one per 16-bit dtype (scale x groups beyond the static exponent window)
    ("win_bf16_per_row_n4096_d64", "bf16", 64, 4, 8, 8, 4096, 4096, 1024, 0, dict(causal=True, scale=80.0)),
    ("win_f16_per_row_n4096_d128", "f16", 128, 4, 8, 8, 4096, 4096, 256, 0, dict(causal=True, scale=16.0)),
    ("win_f32_n4096_d64", "f32", 64, 4, 8, 8, 4096, 4096, 1024, 0, dict(causal=True)),
    # B = 1 long context: the "small" grid forms (key-split forward and dQ, query-split dK/dV)
    ("win_bf16_small_b1h2_n8192_d64", "bf16", 64, 1, 2, 2, 8192, 8192, 1024, 0, dict(causal=True)),
    ("win_bf16_small_b1h4_n8192_d128", "bf16", 128, 1, 4, 4, 8192, 8192, 4096, 0, dict(causal=True)),
]

# ---- packed: id, dtype, D, H, Hk, query lengths, key lengths (None: the query lengths), (left, right), kwargs, max_seqlen (None: exact) --
# numpy.random.default_rng(0).integers(256, 4097, size=32), as tools/varlen_ab.py draws them (72951 tokens, longest 3984)
RAGGED32 = [3523, 2702, 2219, 1292, 1438, 413, 544, 319, 929, 3379, 2750, 3761, 2190, 2586, 3984, 3057, 2684, 2344, 2406, 3847, 1321, 3389,
            2832, 266, 1769, 3549, 2385, 385, 3193, 3058, 3507, 930]
# one 16384-row document among 40 short ones: empty and one-row spans, lengths of t - 1, t, t + 1 around the tile sizes, 1 mod 256
_SHORT = [16, 0, 1, 257, 64, 0, 127, 128, 129, 513, 1, 300, 31, 255, 256, 0, 77, 1, 640, 65]
LONG_DOC = _SHORT + [16384] + [(n * 3 + 5) % 700 for n in _SHORT]
CROSS_Q = [4096, 1, 0, 257, 3000, 130, 2049, 700]
CROSS_K = [2500, 300, 64, 0, 3000, 4000, 513, 1]

PACKED_CASES = [
    ("packed_bf16_d64_ragged32_causal", "bf16", 64, 8, 8, RAGGED32, None, (-1, -1), dict(causal=True), None),
    ("packed_bf16_d128_ragged32_gqa_causal", "bf16", 128, 8, 2, RAGGED32, None, (-1, -1), dict(causal=True), 4096),
    ("packed_bf16_d64_equal_4x4096_causal", "bf16", 64, 8, 8, [4096] * 4, None, (-1, -1), dict(causal=True), None),
    ("packed_bf16_d128_long_doc_causal", "bf16", 128, 4, 2, LONG_DOC, None, (-1, -1), dict(causal=True), None),
    ("packed_f16_d64_long_doc_gqa", "f16", 64, 8, 2, LONG_DOC, None, (-1, -1), dict(causal=True), 20000),
    ("packed_f16_d128_cross_noncausal", "f16", 128, 4, 2, CROSS_Q, CROSS_K, (-1, -1), dict(), None),
    ("packed_bf16_d64_ragged32_w1024", "bf16", 64, 8, 4, RAGGED32, None, (1024, 0), dict(causal=True), 4096),
    ("packed_f32_d64_long_doc_w1024", "f32", 64, 2, 1, LONG_DOC, None, (1024, 0), dict(causal=True), None),
]

# ---- decode: id, dtype, D, B, H, Hk, N, capacity, page (0: contiguous), cache_seqlens before the append, appended keys, (left, right), kw -
CAP = 32768


def ragged_lens(B, n_new):
    """cache_seqlens over {capacity - N_new, capacity - 1 - N_new, 4097, 1, 0}, the full cache first"""
    return [(CAP - n_new, CAP - 1 - n_new, 4097, 1, 0)[b % 5] for b in range(B)]


DECODE_CASES = [
    ("dec_bf16_b1_n1_contig", "bf16", 128, 1, 32, 8, 1, CAP, 0, [CAP - 1], 1, (-1, -1), dict(causal=True)),
    ("dec_bf16_b8_n1_contig_w4096", "bf16", 128, 8, 32, 8, 1, CAP, 0, ragged_lens(8, 1), 1, (4096, 0), dict(causal=True)),
    ("dec_bf16_b8_n5_contig", "bf16", 128, 8, 32, 8, 5, CAP, 0, ragged_lens(8, 5), 5, (-1, -1), dict(causal=True)),
    ("dec_bf16_b8_n1_page16", "bf16", 128, 8, 32, 8, 1, CAP, 16, ragged_lens(8, 1), 1, (-1, -1), dict(causal=True)),
    ("dec_bf16_b8_n5_page256_w4096", "bf16", 128, 8, 32, 8, 5, CAP, 256, ragged_lens(8, 5), 5, (4096, 0), dict(causal=True)),
    ("dec_bf16_b1_n5_page256", "bf16", 128, 1, 32, 8, 5, CAP, 256, [CAP - 5], 5, (-1, -1), dict(causal=True)),
    # an append that crosses a page edge: positions 4094 ... 4098 (page 16 and page 256 both end at 4096) and 253 ... 257
    ("dec_f16_b8_n5_page16_append_crosses", "f16", 128, 8, 32, 8, 5, CAP, 16, [4094, 253, CAP - 5, 14, 0, 4097, 1, 30000], 5, (-1, -1), dict(causal=True)),
    ("dec_f16_b8_n5_page256_append_crosses_w4096", "f16", 128, 8, 32, 8, 5, CAP, 256, [4094, 253, CAP - 5, 14, 0, 4097, 1, 30000], 5, (4096, 0), dict(causal=True)),
    ("dec_f16_b8_n1_contig_two_sided", "f16", 128, 8, 32, 8, 1, CAP, 0, ragged_lens(8, 0), 0, (4096, 100), dict()),
    ("dec_f16_b1_n1_page16_w4096", "f16", 128, 1, 32, 8, 1, CAP, 16, [CAP - 1], 1, (4096, 0), dict(causal=True)),
    ("dec_f32_b8_n5_page256", "f32", 128, 8, 32, 8, 5, CAP, 256, ragged_lens(8, 5), 5, (4096, 0), dict(causal=True)),
    ("dec_bf16_b8_n1_single_kv_head", "bf16", 128, 8, 32, 1, 1, CAP, 0, ragged_lens(8, 1), 1, (-1, -1), dict(causal=True)),
]


def window_line(c):
    name, dtype, D, B, H, Hk, N, M, left, right, kw = c
    return recorder_line(dtype, D, B, H, Hk, N, M, left, right, kw)


def packed_line(c):
    name, dtype, D, H, Hk, lq, lk, (left, right), kw, mx = c
    lk = lq if lk is None else lk
    return recorder_line(dtype, D, len(lq), H, Hk, mx or max(lq), mx or max(lk), left, right, kw, tail=f" varlen {len(lq)} {sum(lq)} {sum(lk)}")


def decode_line(c):
    name, dtype, D, B, H, Hk, N, cap, page, lens, n_new, (left, right), kw = c
    return recorder_line(dtype, D, B, H, Hk, N, cap, left, right, kw, tail=f" decode {cap} {page} {n_new}")


def all_lines():
    """[(case id, the window recorder's input line)] of every case of this file"""
    return [(c[0], window_line(c)) for c in WINDOW_CASES] + [(c[0], packed_line(c)) for c in PACKED_CASES] + \
        [(c[0], decode_line(c)) for c in DECODE_CASES]



# ---- test_gpu_address_range.py: the same call far from its tensor's base and on compact data ------------------------------------------------
# paged pools in vLLM's [num_blocks, page, Hk, D] layout: (dtype, blocks, block ids of the 2 / 4 (/ 8) GiB lines)
ADDR_PAGE, ADDR_HK, ADDR_H, ADDR_D = 256, 8, 32, 128
ADDR_POOLS = [("bf16", 9216, (4096, 8192)), ("f32", 8200, (2048, 4096, 8192))]


def addr_pool_table(nb, lines):
    """three sequences of four blocks: block 0, the blocks on both sides of every line, the last block; sequence 0 ends in the last
    block (an append there lands beyond every line), sequence 1's blocks 2 / 3 are the last but one and block 1 (an append across them)"""
    t = [[lines[-1], 0, lines[0] - 1, nb - 1], [lines[0], lines[-1] - 1, nb - 2, 1],
         [lines[-1] + 1, 2, lines[1] - 1, lines[1]] if len(lines) > 2 else [lines[-1] + 1, 2, 3, 4]]
    assert len({b for row in t for b in row}) == 12
    return t


# N, appended keys, cache_seqlens before the append, window, kwargs
ADDR_POOL_CALLS = [(1, 1, [1023, 767, 300], (-1, -1), dict(causal=True)), (5, 5, [1019, 766, 0], (512, 0), dict(causal=True))]
ADDR_CONTIG = dict(B=72, step=35, cap=32768, lens=[32767, 4097, 32767])      # sequences 0, 35, 70 of a [72, 8, 32768, 128] bf16 cache
# packed [total, 32, 128] bf16 beyond 4 GiB: sequence 64 straddles the line, the last ones lie beyond it
ADDR_PACKED = [8000] + [8192] * 70 + [5000, 3001, 1, 129]
ADDR_PACKED_CHECK = (0, 64, len(ADDR_PACKED) - 2, len(ADDR_PACKED) - 1)
ADDR_DENSE = (72, 32, 8192, 128, (1024, 0))
PITCH = 1 << 20      # row pitch in bytes of the 32-bit tile offset tests
# dense windowed at the pitch: rows, D, (left, right), kwargs -- k_lo x pitch starts beyond 1, 2 and 4 GiB from the slice base
ADDR_PITCH_DENSE = [
    (2304, 64, (300, 0), dict(causal=True)),
    (4608, 128, (300, 200), dict(l2norm_qk=False, scale=0.125)),
    (4608, 64, (300, 0), dict(causal=True, l2norm_qk=False, scale=0.125)),
    (2304, 128, (300, 200), dict()),
]
ADDR_PITCH_PACKED = [1100, 1000, 2100, 300]      # sequences that begin beyond 1, 2 and 4 GiB
ADDR_PITCH_DECODE = dict(cap=4608, lens=[4600], N=5, n_new=5)
ADDR_PITCH_FWD3 = (256, 2304)      # heads inside one row pitch, rows: a chip-filling D = 128 grid that fwd3_kernel takes when contiguous


def address_lines():
    """[(id, window-recorder line)] of the address-range problems: the far and the compact call of each share one line by construction"""
    out = []
    for dtype, nb, _ in ADDR_POOLS:
        for N, n_new, lens, (left, right), kw in ADDR_POOL_CALLS:
            out.append((f"addr_paged_{dtype}_n{N}", recorder_line(dtype, ADDR_D, 3, ADDR_H, ADDR_HK, N, 4 * ADDR_PAGE, left, right, kw,
                                                                  tail=f" decode {4 * ADDR_PAGE} {ADDR_PAGE} {n_new}")))
    out.append(("addr_contiguous_cache", recorder_line("bf16", ADDR_D, 3, ADDR_H, ADDR_HK, 1, ADDR_CONTIG["cap"], -1, -1, dict(causal=True),
                                                       tail=f" decode {ADDR_CONTIG['cap']} 0 1")))
    for name, lens in (("addr_packed_whole", ADDR_PACKED), ("addr_packed_alone", [ADDR_PACKED[s] for s in ADDR_PACKED_CHECK])):
        out.append((name, recorder_line("bf16", 128, len(lens), 32, 32, max(lens), max(lens), -1, -1, dict(causal=True),
                                        tail=f" varlen {len(lens)} {sum(lens)} {sum(lens)}")))
    B, H, N, D, (left, right) = ADDR_DENSE
    out.append(("addr_window_dense_whole", recorder_line("bf16", D, B, H, H, N, N, left, right, dict(causal=True))))
    out.append(("addr_window_dense_slice", recorder_line("bf16", D, 1, 1, 1, N, N, left, right, dict(causal=True))))
    for rows, D, (left, right), kw in ADDR_PITCH_DENSE:
        out.append((f"addr_pitch_dense_n{rows}_d{D}", recorder_line("bf16", D, 1, 1, 1, rows, rows, left, right, kw)))
    for left in (-1, 300):
        out.append((f"addr_pitch_packed_w{left}", recorder_line("bf16", 64, len(ADDR_PITCH_PACKED), 1, 1, max(ADDR_PITCH_PACKED), max(ADDR_PITCH_PACKED),
                                                               left, 0 if left >= 0 else -1, dict(causal=True),
                                                               tail=f" varlen {len(ADDR_PITCH_PACKED)} {sum(ADDR_PITCH_PACKED)} {sum(ADDR_PITCH_PACKED)}")))
        c = ADDR_PITCH_DECODE
        out.append((f"addr_pitch_decode_w{left}", recorder_line("bf16", 128, 1, 4, 1, c["N"], c["cap"], left, 0 if left >= 0 else -1, dict(causal=True),
                                                               tail=f" decode {c['cap']} 0 {c['n_new']}")))
    return out
