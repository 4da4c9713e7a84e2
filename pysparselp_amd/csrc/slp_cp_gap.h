// slp_cp_gap.h -- the scalar arithmetic of the duality-gap certificate the Chambolle-Pock list solver (slp_cp_many.hip) and the
// batched one (slp_cp_batch.hip) stop on, and the NaN-propagating max / min of every per-LP stopping test.  No HIP include: the
// same text compiles for the device and, with an empty SLP_HD, under a host compiler (tests/host/cp_gap_decide_main.cpp pins it
// against tests/cp_gap_cpu.py).  What the kernels add around it is where the numbers come from and the order of the two sums.
#pragma once

#if defined(__HIPCC__)
#define SLP_HD __host__ __device__ __forceinline__
#else
#define SLP_HD inline
#endif

namespace slp {

// max / min as np.max / np.minimum: a NaN on either side stays
SLP_HD double nan_max(double m, double d) { return (d > m || d != d) ? d : m; }
SLP_HD double nan_min(double a, double b) { return (b < a || b != b) ? b : a; }

// column j's term of the bound, d = c + K^T y; the guard keeps 0 * inf out (a free variable whose d is exactly 0)
SLP_HD double cp_gap_col_term(double d, double lb, double ub) { return d != 0.0 ? nan_min(d * lb, d * ub) : 0.0; }

// row r's term of the bound; a row without a finite side has y = 0 and b = inf
SLP_HD double cp_gap_row_term(double y, double b) { return y != 0.0 ? y * b : 0.0; }

// the violation so far (folded from 0) with v = (K x)_r - b_r of one more row
SLP_HD double cp_gap_violation(double so_far, double v, bool equality) { return nan_max(so_far, equality ? __builtin_fabs(v) : v); }

// bound = cols - sy; stop iff violation <= tol_feas and |primal - bound| <= tol_gap (1 + |primal| + |bound|) with a finite
// left-hand side: false for a NaN, and an infinite gap (bound = -inf) never stops, whatever tol_gap * inf would say
SLP_HD bool cp_gap_decide(double primal, double cols, double sy, double violation, double tol_gap, double tol_feas, double *bound_out) {
    const double bound = cols - sy, gap = __builtin_fabs(primal - bound);
    *bound_out = bound;
    return violation <= tol_feas && gap < __builtin_inf() && gap <= tol_gap * (1.0 + __builtin_fabs(primal) + __builtin_fabs(bound));
}

}  // namespace slp

#undef SLP_HD
