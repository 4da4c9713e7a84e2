// slp_cp_shared.h -- the arithmetic of one Chambolle-Pock iteration in SLP_ORDER_SEQUENTIAL, per column and per row, shared by the
// kernels that give a lane a whole column / row: the batched solver (slp_cp_batch.hip: B instances of one K) and the set solver
// (slp_cp_many.hip: one workgroup per LP).  The expressions and the single-accumulator order are those of k_cp_primal<1> /
// k_cp_dual<1> (slp_cp.hip) and of the reference (ChambollePockPPD.py:198-240,:333-342); what differs between the callers is where
// the vectors lie (`stride` between the elements of one instance) and how they are loaded (`LD`).
#pragma once
#include "slp_kernels.h"

namespace slp {

// how a kernel reads an iterate
struct CpLoadPlain {  // written by an earlier launch, or in LDS
    __device__ __forceinline__ double operator()(const double *p) const { return *p; }
};
struct CpLoadWorkgroup {  // global memory written by other lanes of this workgroup before the last barrier (as k_admmb_tile)
    __device__ __forceinline__ double operator()(const double *p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};

// entries s <= q < e of a column of K (a row of K^T) times y: storage order, the terms of rows below `m_eq` in *se, the others in
// *si (row_dot_split<1>); loads four entries ahead, adds in order
template <class LD>
__device__ __forceinline__ void cp_column_sums(i64 s, i64 e, const i32 *__restrict__ tidx, const double *__restrict__ tval, const double *__restrict__ y,
                                               i64 stride, i32 m_eq, LD ld, double *se_out, double *si_out) {
    double se = 0.0, si = 0.0;
    for (i64 q0 = s; q0 < e; q0 += 4) {
        i32 r[4];
        double a[4], g[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const i64 qq = (q0 + q < e) ? q0 + q : e - 1;
            r[q] = tidx[qq];
            a[q] = tval[qq];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) g[q] = ld(y + (i64)r[q] * stride);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q0 + q < e) {
                const double p = a[q] * g[q];
                if (r[q] < m_eq) se += p;
                else si += p;
            }
    }
    *se_out = se;
    *si_out = si;
}

// entries s <= q < e of a row of K times z: storage order, one accumulator (row_dot<1>)
template <class LD>
__device__ __forceinline__ double cp_row_sum(i64 s, i64 e, const i32 *__restrict__ idx, const double *__restrict__ val, const double *__restrict__ z,
                                             i64 stride, LD ld) {
    double kz = 0.0;
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
        for (int q = 0; q < 4; ++q) g[q] = ld(z + (i64)j[q] * stride);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q0 + q < e) kz += a[q] * g[q];
    }
    return kz;
}

// cp_row_sum with a second chain beside it: K z and K x of one row in one walk, each a single accumulator in storage order
// (the certificate's check iteration in slp_cp_many.hip)
template <class LD>
__device__ __forceinline__ void cp_row_sums2(i64 s, i64 e, const i32 *__restrict__ idx, const double *__restrict__ val, const double *__restrict__ z,
                                             const double *__restrict__ x, LD ld, double *kz_out, double *kx_out) {
    double kz = 0.0, kx = 0.0;
    for (i64 q0 = s; q0 < e; q0 += 4) {
        i32 j[4];
        double a[4], g[4], h[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const i64 qq = (q0 + q < e) ? q0 + q : e - 1;
            j[q] = idx[qq];
            a[q] = val[qq];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            g[q] = ld(z + j[q]);
            h[q] = ld(x + j[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q0 + q < e) {
                kz += a[q] * g[q];
                kx += a[q] * h[q];
            }
    }
    *kz_out = kz;
    *kx_out = kx;
}

// d = (c + y_eq * a_eq) + y_ineq * a_ineq (:206,216), or the form of an LP with one kind of rows
__device__ __forceinline__ double cp_direction(double cj, double se, double si, bool has_eq, bool has_ineq) {
    if (has_eq && has_ineq) return (cj + se) + si;
    if (has_eq) return cj + se;
    return cj + si;
}

// x+ = clip(x - T d) (:220-222), z = (1 + theta) x+ - theta x (:226)
__device__ __forceinline__ void cp_primal_point(double d, double xo, double tj, double l, double u, double one_plus_theta, double theta,
                                                double *x2_out, double *z_out) {
    double x2 = xo - tj * d;
    x2 = cp_clip(x2, l, u);
    *z_out = one_plus_theta * x2 - theta * xo;
    *x2_out = x2;
}

// y+ = y + Sigma (K z - b) (:235,240,:334,339), clamped at 0 on an inequality row (:341)
__device__ __forceinline__ double cp_dual_point(double kz, double bi, double yi, double sig, bool ineq) {
    const double r = kz - bi;
    double yn = yi + sig * r;
    if (ineq) yn = (yn < 0.0) ? 0.0 : yn;
    return yn;
}

}  // namespace slp
