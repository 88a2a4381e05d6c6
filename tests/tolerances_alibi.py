"""Bars of the `flash_cosine_sim_attention_alibi` GPU tests (test_gpu_alibi_train.py) that differ from tests/tolerances.py, in one place.

Every comparison of that file uses the existing bars with the bias in the float64 reference, and every class but one stays inside them
(profiles/alibi_train_tolerance_margins.txt: bfloat16 and float16 at or below the attn_bias route, float32 level with it).

The class with a bar of its own: the forward's ELEMENTWISE excess in the per-row-shift regime (scale x groups beyond the static window: 80
in the case table), bfloat16 against exact math on the 16-bit operands and float32 against the raw inputs.  Softmax rows are peaked there,
and a row whose two best keys nearly tie turns a logit error of a few ulps into a visible change of o; among the 30 query heads x 300 rows
of the single-K/V-head cases such rows occur.  The error is a property of those inputs, not of the slopes' kernels: the route that existed
before -- `flash_cosine_sim_attention(..., attn_bias = band + the materialised ALiBi matrix)`, run on the same inputs and judged against
the same float64 reference (tools/alibi_train_margins.py) -- measures the same figure on the slice where the new call is worst (a slice
with zero slopes, in the bfloat16 case), and larger ones elsewhere (bfloat16 up to 6.89e-2, on a slice where the new call has 1.74e-2):

                 new call, worst slice    attn_bias route, same slice   existing bar
    bfloat16     2.987e-2                 2.981e-2                      2.0e-2      (bf16_d32_tail_per_row_w200_-1_full_h30k1_n257m300[0,0])
    float32      5.073e-5                 5.073e-5                      1.6e-5      (f32_d128_full_per_row_w200_-1_full_h30k1_n300m300[7,0])
    float16      7.82e-4                  7.82e-4                       2.5e-3      (inside the existing bar: no entry)

The bar is the attn_bias route's figure ON THAT SLICE times the project's margin of 1.5 (README, tolerances.py) -- not that route's worst
over the class, which would be 2.3 times wider for bfloat16, and never a figure of the new kernels.  rel-L2 of the same outputs and every
gradient of the same cases keep the existing bars.
"""
# dtype -> bar of the forward's elementwise excess in the per-row-shift regime (used where it is above the existing bar)
PER_ROW_FWD_EXCESS = {"bf16": 1.5 * 2.981e-2, "f32": 1.5 * 5.073e-5}
