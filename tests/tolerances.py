"""The stated tolerances of the GPU parity tests, in ONE place, and a measurement log.

Bars (round 5: tightened to <= 1.5x what the kernels measure over the whole GPU suite -- profiles/r05_tolerance_margins.txt lists the
worst measured value of every class next to its bar).  rel-L2 = ||got - ref|| / ||ref||.

    forward o, elementwise  |got - ref| <= atol (* max|v| where stated) + rtol * |ref|,   and   rel-L2 of the whole output
    gradients (dq, dk, dv; d_bias x 1.5)  rel-L2

bf16 keeps 8 significant bits: rounding the OUTPUT alone is 1.1e-3 ... 1.6e-3 rel-L2, so north_star's "within 1e-3 rel." is below what any
bf16 result can reach (README, first screen); f16 and f32 meet it.

`check(label, dtype, measured, bar)` is what every comparison goes through: it returns measured <= bar and, when FCSA_TOL_LOG names a
file, appends one JSON line per comparison (tools/tolerance_margins.py reduces the log to the table in profiles/).
"""
import json
import os

#            atol,  rtol (one output ulp), rel-L2 of the forward output
# Round 5 calibration (profiles/r05_tolerance_margins.txt, all 1331 GPU tests logged): worst measured over the suite ->
#   forward rel-L2   bf16 4.09e-3 (x_n200_d16_causal: D = 16, 200 keys)   f16 5.74e-4   f32 2.13e-6
#   forward excess   bf16 0.75 of the bar   f16 1.56e-3 (of 5e-3)   f32 6.3e-6 (of 2e-5)
#   gradient rel-L2  bf16 5.8e-3 (K28 D = 16 causal; 5.2e-3 on the reference grid)   f16 9.0e-4   f32 2.0e-6 (2.4e-5 at scale 120, its own bar)
# (rounds 1 - 4: bf16 gradients 1.2e-2, f16 3e-3 / forward 5e-3 abs, 1e-3 rel -- 2 - 3x what the kernels do; a regression that doubled
#  the gradient error would have passed)
FWD_TOL = {"f16": (2.5e-3, 2.0 ** -10, 8.5e-4), "bf16": (2e-2, 2.0 ** -7, 4.5e-3), "f32": (1e-5, 2e-5, 4e-6)}
GRAD_TOL = {"f16": 1.4e-3, "bf16": 8.5e-3, "f32": 2e-5}
# the split-key / split-query forms sum partial f32 slabs of a FEW keys / queries each: their bf16 gradients measured 7.7e-3 on the
# smallest splits (tests/test_gpu_split_forward.py), f16 / f32 like everywhere else
SPLIT_GRAD_FACTOR = {"f16": 1.0, "bf16": 1.4, "f32": 1.0}

# float32 in the per-row-shift regime (scale x groups > 75): the forward's elementwise atol times max(1, scale x groups / 64), the factor
# test_gpu_online_reference.py applies there -- a logit of magnitude L carries ~2^-24 L into the exponent.  Measured on the packed-sequence
# forms at scale x groups = 80 (test_gpu_varlen.py::test_varlen_forms): up to 1.28e-5 against the plain 1e-5, each sequence's packed
# output bit-identical to the dense call on that sequence alone; worst 1.13e-5 of the 1.25e-5 this gives on the committed case table.
def f32_per_row_excess_factor(scale, groups):
    return max(1.0, abs(scale) * groups / 64.0)


_LOG = os.environ.get("FCSA_TOL_LOG")


def check(label, dtype, measured, bar, case=None):
    measured, bar = float(measured), float(bar)
    if _LOG:
        with open(_LOG, "a") as f:
            f.write(json.dumps({"label": label, "dtype": str(dtype), "measured": measured, "bar": bar, "case": case}) + "\n")
    return measured <= bar
