"""Bars of the attention-state tests (return_lse, merge_attention_states, the shared-prefix step), by the rule of tests/tolerances.py:
measured bars are 1.5x (or less) the worst value over the new GPU tests; profiles/decode_lse_margins.txt lists every class's worst value
next to its bar.

LSE, two comparisons (tests/lse_reference.py):
  * against float64 on the RAW inputs the bar is DERIVED, lse_reference.derived_lse_bound: 2 u |scale| groups + 1e-4 (6.3e-2 for bfloat16
    at scale 8; measured there: 8.6e-3);
  * against float64 on the rounded operands (16-bit) or the raw inputs (float32) what is left is float32 accumulation, the exponential's
    approximation, one float32 rounding of the result (9.5e-7 is one ulp of an LSE of 8 ... 16) and, for the 16-bit types, the few elements
    of k^ that the kernel's float32 normalisation rounds to the other neighbour than the float64 one: LSE_TOL below, measured.  The 16-bit
    values sit at 0.14 % (bfloat16) and 1.1 % (float16) of the derived bound: a value anywhere near that bound would be a bug.
The merge kernel against float64 on its own inputs: o by the derived bar u |ref| + 2^-20 max_s |o_s| (half an output ulp and eight
float32 ulps), lse by MERGE_LSE_TOL, measured (5.8e-7: one float32 ulp of an LSE of 4 ... 8).
Composed routes (one attention over two or three calls; the shared-prefix step) round the partial outputs once more before the merge:
COMPOSED_FWD_TOL are their forward bars (atol, rtol, rel-L2; the parity policy of test_gpu_kvcache._verify), measured next to the single
call's values on the same inputs -- bfloat16 rel-L2 4.00e-3 composed against 3.55e-3 single, float16 4.81e-4 against 4.09e-4, float32
4.02e-7 against 4.03e-7; the composed error stayed within 1.27x the single call's on every case (the tests assert 2x)."""

#          |lse - ref| on the operands the kernel is fed           worst measured
LSE_TOL = {"bf16": 1.33e-4, "f16": 9.5e-5, "f32": 1.4e-6}        # 8.85e-5   8.53e-5   9.33e-7
MERGE_LSE_TOL = 8.8e-7                                           # 5.82e-7
#                    atol (worst excess)  rtol (one output ulp)  rel-L2 (worst)
COMPOSED_FWD_TOL = {"f16": (7.2e-4, 2.0 ** -10, 7.1e-4),         # 4.83e-4                4.81e-4
                    "bf16": (4.4e-3, 2.0 ** -7, 5.0e-3),         # 3.32e-3                4.00e-3  (1.25x: the single call's bar is 4.5e-3)
                    "f32": (3.2e-7, 2e-5, 6.0e-7)}               # 2.17e-7                4.02e-7
