// slp_admm_gap.h -- the scalar rule that makes an ADMM multiplier usable in the duality-gap certificate of the two single ADMM
// solvers (slp_admm.hip, slp_admm_cg.hip; include/slp_hip_ext_admm_gap.h).  No HIP include, like slp_cp_gap.h, which it
// builds on: the same text compiles for the device and, with an empty SLP_HD, under a host compiler (tests/host/admm_gap_dual_main.cpp pins it against
// tests/admm_gap_cpu.py).
//
// A slack column j (cost 0, one stored entry a in row i) has d_j = a * y_i, so its term of the bound is min(d_j lb_j, d_j ub_j):
// -inf as soon as y_i pushes the slack towards a side it has no bound on.  An ADMM multiplier does that freely.  Any y gives a
// valid bound, so the certificate uses y_i = 0 on such a row and lam_i elsewhere.
#pragma once

#include "slp_cp_gap.h"

#if defined(__HIPCC__)
#define SLP_HD __host__ __device__ __forceinline__
#else
#define SLP_HD inline
#endif

namespace slp {

// would the slack column with entry a and box [lb, ub] contribute -inf under the multiplier lam?  (one product a * lam, then the
// two of the column term; a NaN anywhere answers no, and the NaN then shows in the bound)
SLP_HD bool admm_gap_slack_unbounded(double a, double lam, double lb, double ub) {
    const double p = a * lam;
    return p != 0.0 && nan_min(p * lb, p * ub) == -__builtin_inf();
}

// the multiplier the certificate uses on a row: 0 where one of the row's slack columns answered yes
SLP_HD double admm_gap_dual(double lam, bool repaired) { return repaired ? 0.0 : lam; }

}  // namespace slp

#undef SLP_HD
