// slp_admm_iter.h -- the arithmetic of one ADMM iteration with the projected Gauss-Seidel x-step in SLP_ORDER_SEQUENTIAL, per
// column / per row of M / per row of A, shared by the kernels that give a lane a whole row: the batched solver
// (slp_admm_batch.hip: B instances of one structure) and the list solver (slp_admm_many.hip: one workgroup per LP).  The
// expressions and the single-accumulator order are those of k_admm_rhs<1> / k_gs_level<true> / k_admm_multiplier<1>
// (slp_admm.hip) and of the reference (ADMM.py:148, gaussSiedel.pyx:131-152, ADMM.py:261-263); what differs between the callers
// is where the vectors lie (STRIDE between the elements of one instance) and how they are loaded (LD).  As slp_cp_shared.h.
#pragma once
#include "slp_kernels.h"

namespace slp {

// a value another lane of the workgroup may have stored before the last barrier: never kept in a register across it
#ifndef SLP_ADMMB_SCOPE
#define SLP_ADMMB_SCOPE __HIP_MEMORY_SCOPE_WORKGROUP
#endif

// how a kernel reads an iterate
struct AdmmLoadPlain {  // in LDS (the barrier orders it), or written by an earlier launch
    __device__ __forceinline__ double operator()(const double *p) const { return *p; }
};
struct AdmmLoadWorkgroup {  // global memory written by other lanes of this workgroup before the last barrier
    __device__ __forceinline__ double operator()(const double *p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, SLP_ADMMB_SCOPE); }
};

// sum_q val[q] * v[idx[q] * STRIDE] over s <= q < e: storage order, one accumulator; loads four entries ahead (row_dot<1>)
template <int STRIDE, class LD>
__device__ __forceinline__ double admm_dot(i64 s, i64 e, const i32 *__restrict__ idx, const double *__restrict__ val, const double *v, LD ld) {
    double acc = 0.0;
    for (i64 q0 = s; q0 < e; q0 += 4) {
        i32 j[4];
        double a[4], g[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const i64 qq = (q0 + q < e) ? q0 + q : e - 1;
            j[q] = idx[qq];
            a[q] = val[qq];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) g[q] = ld(v + (i64)j[q] * STRIDE);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q0 + q < e) acc += a[q] * g[q];
    }
    return acc;
}

// y_j = ((q_j + gamma_ineq xp_j) - (A^T lambda)_j) - 0 over the entries s .. e of row j of A^T (:148).  qj, xpj: where q_j and xp_j
// lie, read after the walk; xp_is_x: xp_j is the iterate itself (loaded as one), else the start's max(x0, 0)
template <int STRIDE, class LD>
__device__ __forceinline__ double admm_rhs_one(i64 s, i64 e, const i32 *__restrict__ tidx, const double *__restrict__ tval, const double *lam,
                                               const double *qj, const double *xpj, bool xp_is_x, double gamma_ineq, LD ld) {
    const double atl = admm_dot<STRIDE>(s, e, tidx, tval, lam, ld);
    const double xp = xp_is_x ? ld(xpj) : *xpj;
    return (*qj + gamma_ineq * xp) - atl;
}

// the new x_i from the entries s .. e of row i of M's level-ordered copy: y_i = bi, the old x_i = xi, 1 / M_ii = inv, clamped to [l, u]
template <int STRIDE, class LD>
__device__ __forceinline__ double admm_sweep_one(i64 s, i64 e, const i32 *__restrict__ gidx, const double *__restrict__ gval, const double *x,
                                                 double bi, double xi, double inv, double l, double u, LD ld) {
    double v = admm_dot<STRIDE>(s, e, gidx, gval, x, ld);
    v = (bi - v) * inv + xi;  // gaussSiedel.pyx:145 with w = 1
    if (v < l) v = l;         // :148-151
    else if (v > u) v = u;
    return v;
}

// lambda_i + gamma_eq ((A x)_i - b_i) over the entries s .. e of row i of A (:261-263).  li, bi: where lambda_i and b_i lie, read
// after the walk
template <int STRIDE, class LD>
__device__ __forceinline__ double admm_mult_one(i64 s, i64 e, const i32 *__restrict__ aidx, const double *__restrict__ aval, const double *x,
                                                const double *li, const double *bi, double gamma_eq, LD ld) {
    const double ax = admm_dot<STRIDE>(s, e, aidx, aval, x, ld);
    return ld(li) + gamma_eq * (ax - *bi);
}

// admm_mult_one that also hands out the residual (A x)_i - b_i it forms, for a caller that tests it (the stopping test of
// slp_admm_many.hip): one walk, the same expressions, so lambda_i keeps its bits
template <int STRIDE, class LD>
__device__ __forceinline__ double admm_mult_res_one(i64 s, i64 e, const i32 *__restrict__ aidx, const double *__restrict__ aval, const double *x,
                                                    const double *li, const double *bi, double gamma_eq, LD ld, double *res) {
    const double ax = admm_dot<STRIDE>(s, e, aidx, aval, x, ld);
    const double r = ax - *bi;
    *res = r;
    return ld(li) + gamma_eq * r;
}

}  // namespace slp
