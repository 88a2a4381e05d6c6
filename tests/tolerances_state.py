"""Bars of the training-side attention-state tests (tests/test_gpu_state.py), by the rule of tests/tolerances.py: each measured bar is at
most 1.5x the worst value over the new GPU tests; profiles/state_margins.txt lists every class's worst value next to its bar.  The
reference is tests/state_reference.py: float64 torch autograd of <o, do> + <lse, dlse> over the plain composite, on the operands the kernels
are fed for the 16-bit types (operand-faithful) and on the raw inputs for float32.

  lse        two comparisons, as in tests/tolerances_lse.py.  Against float64 on the RAW inputs the bar is derived
             (lse_reference.derived_lse_bound) and asserted as it stands.  Against float64 on the operands it is STATE_LSE_TOL, measured.
             The expectation was tolerances_lse.LSE_TOL (the decode LSE); the 16-bit types need more, and DESIGN.md section 4.9 says why:
             the training forward's row sum is the exact float32 sum of the P~ values ROUNDED to the 16-bit type (DESIGN.md section 5:
             what makes o a true convex combination of V rows), so ln(l) carries one relative rounding u of the type per term -- at most
             u = 3.9e-3 (bfloat16) / 4.9e-4 (float16) for a row with one dominant key, measured 3.2e-3 / 4.7e-4 -- where the decode
             kernel sums un-rounded float32 values.  The lse is consistent with the o and the P of the backward (both normalise by the same
             l).  float32: 2.6e-6 on a D = 128 window of 8 keys (LSE_TOL 1.4e-6 was measured on the decode kernel's 16 rows x 32 keys
             steps; a float32 logit of size 8 from 128 products carries ~ 3 ulps of 9.5e-7).
             Without l2norm_qk the derived bound keeps only 1e-4 ("float32 accumulation and the exponential"), and with it the bound
             falls below u once |scale| groups < 1/2: no room for the rounding of P~ (float16 measured 2.10e-4 against 1.0e-4 on the
             "no-l2norm" case).  There the binding takes the lse from the inv_l of a second, float32 forward (csrc/fcsa_torch.cpp,
             attention_state_forward), and the bound holds as it stands.
  gradients  rel-L2 of dq, dk, dv with a random dlse: STATE_GRAD_TOL (STATE_SPLIT_GRAD_TOL on the split forms).  The expectation is
             tolerances.GRAD_TOL (x SPLIT_GRAD_FACTOR): a gradient for the lse adds one float32 subtraction per row to delta, and every
             bar below stays under it.
  merge      backward of the merge kernel against float64 autograd on its own inputs: d o_s elementwise |err| <= u |ref| + MERGE_DO_ATOL *
             max|do| (half an output ulp and float32 arithmetic), d lse_s by MERGE_DLSE_TOL relative to max(1, max|ref|).
  composed   one attention over 2 or 3 key chunks (and the causal ring schedule) merged by merge_attention_states_with_grad: every error
             is asserted within COMPOSED_FACTOR x the single call's error on the same inputs (the rule of tolerances_lse.py); measured
             at most 1.57x (float16 dq over three chunks), float32 0.96 - 1.03x.
  gradcheck  float32, (1, 1, 5, 7, D 16), scale 2: torch.autograd.gradcheck with the eps and tolerances below -- central differences
             with eps = 1e-2 of float32 kernels carry u / eps ~ 6e-6 of rounding noise per unit of output plus the O(eps^2) truncation."""
import tolerances as T

#                 |lse - ref| on the operands                      worst measured (profiles/state_margins.txt)
STATE_LSE_TOL = {"bf16": 4.8e-3, "f16": 6.9e-4, "f32": 3.9e-6}       # 3.231e-3  4.652e-4  2.616e-6
#                 rel-L2 of dq / dk / dv
STATE_GRAD_TOL = {"bf16": 7.4e-3, "f16": 5.8e-4, "f32": 2.2e-6}      # 4.938e-3  3.874e-4  1.522e-6
STATE_SPLIT_GRAD_TOL = {"bf16": 3.9e-3}                              # 2.636e-3 (split dQ keys x8; split dK/dV queries x8: 2.435e-3)
MERGE_DO_ATOL = 2.0 ** -22                                           # 1.662e-7
MERGE_DLSE_TOL = 1.6e-6                                              # 1.109e-6
COMPOSED_FACTOR = 2.0                                                # 1.574
GRADCHECK = dict(eps=1e-2, atol=2e-3, rtol=2e-3)

assert all(STATE_GRAD_TOL[d] <= T.GRAD_TOL[d] for d in STATE_GRAD_TOL)
assert all(STATE_SPLIT_GRAD_TOL[d] <= T.GRAD_TOL[d] * T.SPLIT_GRAD_FACTOR[d] for d in STATE_SPLIT_GRAD_TOL)
