// slp_admm_many.hip -- ADMM with the projected Gauss-Seidel x-step on a LIST of LPs whose constraint matrices differ: one
// workgroup per LP, whole iterations inside one launch.  No counterpart in the reference (single-threaded numpy: N solves are N
// calls of lp_admm, ADMM.py:47-269).  The x-step of a small LP is a chain of narrow dependency levels -- a chain of barriers on a
// nearly idle chip when it is solved alone -- and N independent LPs are N independent workgroups.  One iteration of an LP, with
// the device functions of slp_admm_iter.h (the arithmetic of slp_admm_batch.hip), in k_admmb_tile's order:
//   right-hand side over the N columns  y_j = ((q_j + gamma_ineq xp_j) - (A^T lambda)_j) - 0              [ADMM.py:148]
//   barrier
//   level by level, a barrier after each  v = (y_i - sum_k x[idx_k] val_k) invd + x_i, clamped            [gaussSiedel.pyx:131-152]
//   multiplier update over the m rows     lambda_i += gamma_eq ((A x)_i - b_i)                             [ADMM.py:261-263]
//   barrier
// xp is max(x0, 0) before the first multiplier step and x afterwards (:98, :259).  Every dot product is one lane, storage order,
// one accumulator: every LP is bit for bit the iterate of slp_admm in SLP_ORDER_SEQUENTIAL on that LP alone.
//
// Set-up.  The chain of slp_admm_create_lp (row scalings, standard form, second scaling, SpGEMM for M, A^T b, level plan) runs
// ONCE, on the block-diagonal composite: the equality rows of all LPs (LP 0, LP 1, ...), then the inequality rows of all LPs; the
// columns of LP k offset by col0[k]; its standard form has all original variables first and all slacks after them.  That keeps
// the relative order of every LP's columns and rows, and every step of the chain is per row, per column, or a product that adds
// in row order (slp_spgemm.hip: the terms of M[i, j] in increasing row of A), so every LP gets the entries, the entry order and
// the values of its own set-up.  The plan is made with earliest_levels (slp_admm_shared.h): the single solver moves sink rows to a
// level of their own when one LP has more than 4096 of them, a rule on the size of the whole system; here it is applied per LP, on
// the host, to the levels of the composite (admmm_regroup), so that every LP has the level count of its own plan.
// After the chain: M's level-ordered copy is regrouped on the device so that every LP's rows are contiguous and in (level, row)
// order inside the LP (the host sees M's row pointer, row order and one flag per row, never its entries); the index arrays of A,
// A^T and M are rewritten to indices local to the LP -- original variables first, then that LP's slacks; equality rows first,
// then that LP's inequality rows: the order of the LP's own standard form; q, xp0, x, lb, ub, c and b are gathered LP by LP.
// AdmmmLp, one per LP, holds its column and row ranges, where its vectors lie, and its level pointer.
//
// Forms, workgroup width and launch cap: slp_many_plan.h (switches SLP_ADMM_MANY_FORM, SLP_ADMM_MANY_KMAX).  Here the lds form
// holds x, y, lambda (2 N + m <= kAdmmmLdsLimit doubles; y is rebuilt by every right-hand side, so only x and lambda are loaded and
// written back; the global form as k_admmb_tile); q, xp0, lb, ub, b and the matrices are read from global memory in both.  A pass
// is the workgroup once over a stage or a level: nlevels + 2 passes per iteration.
//
// Workgroup width W: a launch wants max over its LPs of max(widest level, ceil(max(N, m) / 4)) lanes.  An iteration is
// nlevels + 2 barriers, and a barrier costs with the number of waves that
// meet at it; the levels of small LPs are a few rows wide while N and m reach hundreds, so W follows the widest level, and the
// two full passes (right-hand side, multipliers) are bounded at four trips per lane instead of sizing W by them.  A function of
// the shapes (and M's pattern) only.
// No atomics between workgroups, no spin waits, no grid barrier: a workgroup never waits for another.
//
// Report (:213-248), per LP, one workgroup of 256 lanes on the written-back state: lane t takes rows (columns) t, t + 256, ...
// in increasing order, then block_reduce: a fixed order, a function of the shapes only.  The maxima are exact.
//
// Stopping (slp_many_admm_set_stop; off after create), by the protocol slp_many.h holds once for this file and slp_cp_many.hip:
// the head of the record, entering from it, a wave's slot, lane 0's fold, the decision slot with its barrier, and on the host the
// read-out and the re-arming.  AdmmmCtl, one per LP in device memory: iterations completed, the stopped
// flag, the stopping iteration, the last evaluated residual and step, and the reduced step of a sweep whose multiplier update has
// not run yet.  Iterations of an LP count from 1 over its whole life; at the end of an iteration t with t % check_every == 0 the
// LP stops iff  residual_t = max_i |(A x_t)_i - b_i| <= tol_residual  and  step_t = max_j |x_t,j - x_{t-1},j| <= tol_step: the
// residual is the value the multiplier update forms (admm_mult_res_one; bit for bit column 1 of the report after t iterations),
// the old x_j is the value the sweep loads, and both maxima are NaN-propagating as np.max -- exact in any order, so the decision
// is that of a CPU restatement.  The test is the template parameter STOP of k_admmm_iterate: STOP = false is the kernel without
// it -- no extra barrier, no extra LDS, no word of the control record read or written (the host counts the iterations).  With
// STOP only a check iteration accumulates anything, in loops of its own: a lane its fabs over its rows of all levels and of the
// multiplier pass, then a wave reduces by shuffles into one LDS slot per wave and quantity; after the multiplier pass's barrier
// lane 0 folds the slots, writes the record and ONE LDS slot with the decision, and one more barrier later every lane reads that
// slot: the break is uniform, and so is every barrier.  The sweep's slots are written behind the last level's barrier and read
// behind the multiplier pass's; a sweep-only launch (sweep_step) has no such barrier and adds one, in a check iteration only,
// before lane 0 writes the reduced step into the record, where it waits for multiplier_step.  A stopped LP's workgroup returns
// before its first barrier (the flag was written by an earlier launch: the same for every lane) and its x, lambda are never
// written again; in the launch in which it stops it leaves the loop and, in the lds form, writes them back.  The count of an LP
// is read from the record at the start of a launch, so the stopping iteration does not depend on how a run is split into calls
// and launches.
//
// Compaction (slp_many_admm_set_compaction, include/slp_hip_ext_many_live.h; off after create): the template parameter LIVE of
// k_admmm_iterate<., true, .>, by the text slp_cp_many.hip uses -- ManyFormLive, many_form_call (slp_many_plan.h), ManyFormLists,
// many_form_list, many_form_state (slp_many.h).  With compaction on and the test armed, admmm_run reads the records back at the
// start of a call (one download; it synchronises); per form every launch of the call is preceded by k_many_live for that form and
// runs over as many workgroups as LPs of the form were live when the call began, held to the cap of that many workgroups; a.list
// is the live list, and a workgroup at or past *live_n returns before anything else.  Every LP stays bit for bit.
#include <algorithm>
#include <cmath>
#include <memory>
#include <type_traits>
#include <utility>

#include "slp_kernels.h"
#include "slp_admm_iter.h"
#include "slp_admm_shared.h"
#include "slp_many.h"
#include "../../include/slp_hip_ext_many_live.h"

namespace slp {

constexpr int kAdmmmMaxBlock = 1024;
// doubles of x, y, lambda an LP may hold in LDS: 160 000 of the compute unit's 163 840 bytes (kCpmLdsLimit's reasoning)
constexpr i64 kAdmmmLdsLimit = 20000;
constexpr i64 kAdmmmSinks = 4096;  // gs_plan: more sink rows than this in ONE LP go to a level of their own

struct AdmmmLp {
    i64 col0, slack0;  // first variable column and first slack column in the composite: rows of A^T
    i64 eq0, in0;      // first equality row and first inequality row in the composite: rows of A
    i64 x0;            // where x, y, q, xp0, lb, ub, c and the rows of M's regrouped copy lie (sum of the N before)
    i64 lam0;          // where lambda and b lie (sum of the m before)
    i64 lptr0;         // where its level pointer lies (nlevels + 1 positions, counted from x0)
    i32 n, m_eq, m_in;
    i32 nlevels, widest;
    i32 form;          // 0 lds, 1 global
};

// column j of the LP (variables first, then its slacks) in the composite's order; its rows: many_row
__device__ __forceinline__ i64 admmm_col(const AdmmmLp &lp, i32 j) { return j < lp.n ? lp.col0 + j : lp.slack0 + (j - lp.n); }

// the index arrays of both orientations of A, composite -> local to the LP; one workgroup per LP (as k_cpm_localise)
__global__ __launch_bounds__(kBlock) void k_admmm_localise(const AdmmmLp *__restrict__ lps, const i64 *__restrict__ ptr, i32 *__restrict__ idx,
                                                           const i64 *__restrict__ tptr, i32 *__restrict__ tidx, i64 n_all, i64 m_eq_all) {
    const AdmmmLp lp = lps[blockIdx.x];
    const i32 m = lp.m_eq + lp.m_in, N = lp.n + lp.m_in;
    for (i32 r = threadIdx.x; r < m; r += kBlock) {
        const i64 g = many_row(lp.eq0, lp.in0, lp.m_eq, r);
        for (i64 q = ptr[g]; q < ptr[g + 1]; ++q) {
            const i64 c = idx[q];
            idx[q] = (i32)(c < n_all ? c - lp.col0 : lp.n + (c - lp.slack0));
        }
    }
    for (i32 j = threadIdx.x; j < N; j += kBlock) {
        const i64 g = admmm_col(lp, j);
        for (i64 q = tptr[g]; q < tptr[g + 1]; ++q) {
            const i64 r = tidx[q];
            tidx[q] = (i32)(r < m_eq_all ? r - lp.eq0 : lp.m_eq + (r - lp.in0));
        }
    }
}

// up[t] = 1 when the row at position t of M's level-ordered copy has an entry right of its diagonal (M's pattern is symmetric:
// the coupled_up of gs_plan).  Rows without one, at a level above 0, are the sinks.
__global__ void k_admmm_coupled_up(i64 N, const i64 *__restrict__ gptr, const i32 *__restrict__ gidx, const i32 *__restrict__ grows,
                                   unsigned char *__restrict__ up) {
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < N; t += (i64)gridDim.x * blockDim.x) {
        const i32 i = grows[t];
        unsigned char u = 0;
        for (i64 q = gptr[t]; q < gptr[t + 1]; ++q) u |= (gidx[q] > i) ? 1 : 0;
        up[t] = u;
    }
}

// M's level-ordered copy regrouped LP by LP: new position p holds the row of old position src[p], its entries at nptr[p] ..
// nptr[p + 1] with the indices local to the LP; lp_of[p] is its LP
__global__ void k_admmm_regroup(i64 N, const AdmmmLp *__restrict__ lps, const i32 *__restrict__ lp_of, const i32 *__restrict__ src,
                                const i64 *__restrict__ gptr, const i32 *__restrict__ gidx, const double *__restrict__ gval,
                                const double *__restrict__ ginvd, const i32 *__restrict__ grows, i64 n_all, const i64 *__restrict__ nptr,
                                i32 *__restrict__ nidx, double *__restrict__ nval, double *__restrict__ ninvd, i32 *__restrict__ nrows) {
    for (i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (i64)gridDim.x * blockDim.x) {
        const i64 t = src[p];
        const AdmmmLp lp = lps[lp_of[p]];
        i64 o = nptr[p];
        for (i64 q = gptr[t]; q < gptr[t + 1]; ++q, ++o) {
            const i64 c = gidx[q];
            nidx[o] = (i32)(c < n_all ? c - lp.col0 : lp.n + (c - lp.slack0));
            nval[o] = gval[q];
        }
        const i64 i = grows[t];
        nrows[p] = (i32)(i < n_all ? i - lp.col0 : lp.n + (i - lp.slack0));
        ninvd[p] = ginvd[t];
    }
}

// a vector over the composite's columns (rows) -> LP by LP in the LP's own order; one workgroup per LP
__global__ __launch_bounds__(kBlock) void k_admmm_gather_cols(const AdmmmLp *__restrict__ lps, const double *__restrict__ src,
                                                              double *__restrict__ dst) {
    const AdmmmLp lp = lps[blockIdx.x];
    const i32 N = lp.n + lp.m_in;
    for (i32 j = threadIdx.x; j < N; j += kBlock) dst[lp.x0 + j] = src[admmm_col(lp, j)];
}
__global__ __launch_bounds__(kBlock) void k_admmm_gather_rows(const AdmmmLp *__restrict__ lps, const double *__restrict__ src,
                                                              double *__restrict__ dst) {
    const AdmmmLp lp = lps[blockIdx.x];
    const i32 m = lp.m_eq + lp.m_in;
    for (i32 r = threadIdx.x; r < m; r += kBlock) dst[lp.lam0 + r] = src[many_row(lp.eq0, lp.in0, lp.m_eq, r)];
}

struct AdmmmArgs {
    const AdmmmLp *lps;
    const i32 *list;                                        // the LPs of this launch
    const i64 *tptr; const i32 *tidx; const double *tval;   // rows of A^T, composite row order, local indices
    const i64 *aptr; const i32 *aidx; const double *aval;   // rows of A
    const i64 *gptr; const i32 *gidx; const double *gval; const double *ginvd; const i32 *grows; const i64 *lptr;  // M, regrouped
    const double *b, *q, *c, *lb, *ub, *xp0;
    double *x, *y, *lam;
    double gamma_eq, gamma_ineq;
};

// per LP, in device memory: the head of slp_many.h and what the test evaluates
struct AdmmmCtl : ManyCtl {
    double residual;  // the last evaluated max |A x - b|, +inf before the first test
    double step;      // the last evaluated max |x_t - x_{t-1}|, +inf before the first test
    double dx;        // the sweep's maximum of a check iteration, carried from sweep_step to multiplier_step
};

struct AdmmmStop {
    AdmmmCtl *ctl;
    double tol_residual, tol_step;
    i64 check_every;
};

constexpr int kAdmmmWaves = kAdmmmMaxBlock / kWave;
// per wave the maxima of the sweep and of the multiplier pass, then the decision
constexpr int kAdmmmRed = 2 * kAdmmmWaves + 1;
static_assert(kAdmmmRed * sizeof(double) + kAdmmmLdsLimit * sizeof(double) <= 160 * 1024,
              "the slots of the stopping test and the iterates of the lds form share the compute unit's 160 KiB");

// `iters` times the stages of one LP (bit 0 right-hand side + sweep, bit 1 multiplier); first: xp = xp0 in the first right-hand side.
// STOP: the stopping test of the header comment, by the protocol of slp_many.h; `sp` is not looked at without it.
// LIVE (with STOP only): a.list is the form's live list, which k_many_live wrote in front of this launch, and *live_n its length; a
// workgroup at or past it returns before anything else (*live_n is the same for every lane).  `live_n` is not looked at without it.
template <bool LDS, bool STOP, bool LIVE>
__global__ __launch_bounds__(kAdmmmMaxBlock) void k_admmm_iterate(AdmmmArgs a, int iters, int first, int stages, AdmmmStop sp, const i32 *live_n) {
    static_assert(STOP || !LIVE, "an unarmed state has no stopped LP: no live variant");
    extern __shared__ __attribute__((aligned(16))) double admmm_lds[];
    __shared__ double admmm_red[STOP ? kAdmmmRed : 1];  // unused without STOP: the compiler drops it
    using LD = typename std::conditional<LDS, AdmmLoadPlain, AdmmLoadWorkgroup>::type;
    const LD ld;
    if (LIVE && blockIdx.x >= (unsigned)*live_n) return;
    const i32 id = a.list[blockIdx.x];
    const AdmmmLp lp = a.lps[id];
    const i32 N = lp.n + lp.m_in, m = lp.m_eq + lp.m_in, W = (i32)blockDim.x, tid = (i32)threadIdx.x;
    i64 done = 0, until = 0;  // STOP: iterations completed; iterations up to and including the next check
    if (STOP && !many_enter(sp.ctl + id, sp.check_every, &done, &until)) return;
    double *xg = a.x + lp.x0, *yg = a.y + lp.x0, *lg = a.lam + lp.lam0;
    double *xs = xg, *ys = yg, *ls = lg;
    if (LDS) {
        xs = admmm_lds;
        ys = xs + N;
        ls = ys + N;
        for (i32 j = tid; j < N; j += W) xs[j] = xg[j];  // y is rebuilt by the right-hand side before every sweep: not kept
        for (i32 r = tid; r < m; r += W) ls[r] = lg[r];
        __syncthreads();
    }
    const double *q = a.q + lp.x0, *xp0 = a.xp0 + lp.x0, *lb = a.lb + lp.x0, *ub = a.ub + lp.x0, *b = a.b + lp.lam0;
    const i64 *gptr = a.gptr + lp.x0, *lptr = a.lptr + lp.lptr0;
    const double *ginvd = a.ginvd + lp.x0;
    const i32 *grows = a.grows + lp.x0;
    for (int it = 0; it < iters; ++it) {
        const bool check = STOP && until == 1;  // uniform: a function of the record and of `it`
        if (stages & 1) {
            const bool use_xp0 = first && it == 0;
            for (i32 j = tid; j < N; j += W) {
                const i64 g = admmm_col(lp, j);
                ys[j] = admm_rhs_one<1>(a.tptr[g], a.tptr[g + 1], a.tidx, a.tval, ls, q + j, use_xp0 ? xp0 + j : xs + j, !use_xp0, a.gamma_ineq, ld);
            }
            __syncthreads();
            double dx = 0.0;  // a lane without a row in any level contributes 0.0
            for (i32 l = 0; l < lp.nlevels; ++l) {
                const i64 beg = lptr[l], end = lptr[l + 1];
                if (check) {  // a loop of its own, as in the multiplier pass: the other one stays the loop of the kernel without the test
                    for (i64 t = beg + tid; t < end; t += W) {
                        const i32 i = grows[t];
                        const double yi = ld(ys + i), xi = ld(xs + i);
                        const double v = admm_sweep_one<1>(gptr[t], gptr[t + 1], a.gidx, a.gval, xs, yi, xi, ginvd[t], lb[i], ub[i], ld);
                        xs[i] = v;
                        dx = nan_max(dx, fabs(v - xi));
                    }
                } else {
                    for (i64 t = beg + tid; t < end; t += W) {
                        const i32 i = grows[t];
                        xs[i] = admm_sweep_one<1>(gptr[t], gptr[t + 1], a.gidx, a.gval, xs, ld(ys + i), ld(xs + i), ginvd[t], lb[i], ub[i], ld);
                    }
                }
                __syncthreads();  // same compute unit: the stores of this level are visible to the next one
            }
            // behind the last level's barrier; read behind the multiplier pass's, or behind the one below
            if (check) many_post<1, 1>(admmm_red, kAdmmmWaves, tid, &dx);
        }
        if (STOP && !(stages & 2)) {  // sweep_step: the reduced step waits in the record for multiplier_step
            if (check) {
                __syncthreads();  // the slots of every wave are written
                if (tid == 0) {
                    double dx;
                    many_fold<1, 1>(admmm_red, kAdmmmWaves, W, &dx);
                    sp.ctl[id].dx = dx;
                }
            }
            continue;
        }
        if (stages & 2) {
            if (check) {
                double dr = 0.0;  // 0.0 for an LP without rows, and from a lane without one
                for (i32 r = tid; r < m; r += W) {
                    const i64 g = many_row(lp.eq0, lp.in0, lp.m_eq, r);
                    double res;
                    ls[r] = admm_mult_res_one<1>(a.aptr[g], a.aptr[g + 1], a.aidx, a.aval, xs, ls + r, b + r, a.gamma_eq, ld, &res);
                    dr = nan_max(dr, fabs(res));
                }
                many_post<1, 1>(admmm_red + kAdmmmWaves, kAdmmmWaves, tid, &dr);
            } else {
                for (i32 r = tid; r < m; r += W) {
                    const i64 g = many_row(lp.eq0, lp.in0, lp.m_eq, r);
                    ls[r] = admm_mult_one<1>(a.aptr[g], a.aptr[g + 1], a.aidx, a.aval, xs, ls + r, b + r, a.gamma_eq, ld);
                }
            }
            __syncthreads();
        }
        if (STOP) {  // here an iteration is complete
            ++done;
            if (!check) {
                --until;
                continue;
            }
            until = sp.check_every;
            if (tid == 0) {
                AdmmmCtl *ctl = sp.ctl + id;
                // the sweep's step, the residual.  multiplier_step: the step waited in the record (as in k_cpm_iterate, named up
                // front; the compiler sinks the load into that case)
                double f[2] = {ctl->dx, 0.0};
                if (stages & 1) many_fold<2, 3>(admmm_red, kAdmmmWaves, W, f);
                else many_fold<1, 1>(admmm_red + kAdmmmWaves, kAdmmmWaves, W, f + 1);
                ctl->residual = f[1];
                ctl->step = f[0];
                many_decide(ctl, done, f[1] <= sp.tol_residual && f[0] <= sp.tol_step, admmm_red + 2 * kAdmmmWaves);  // false for a NaN
            }
            if (many_decided(admmm_red + 2 * kAdmmmWaves)) break;  // the one barrier the test adds to a whole iteration
        }
    }
    if (STOP && (stages & 2) && tid == 0) sp.ctl[id].done = done;
    if (LDS) {
        for (i32 j = tid; j < N; j += W) xg[j] = xs[j];
        for (i32 r = tid; r < m; r += W) lg[r] = ls[r];
    }
}

// out[3 k + 0..2] as slp_admm_report; one workgroup per LP
__global__ __launch_bounds__(kBlock) void k_admmm_report(AdmmmArgs a, int first, double *__restrict__ out) {
    __shared__ double lds[kBlock / kWave];
    const AdmmmLp lp = a.lps[blockIdx.x];
    const i32 N = lp.n + lp.m_in, m = lp.m_eq + lp.m_in;
    const double *x = a.x + lp.x0, *lam = a.lam + lp.lam0, *b = a.b + lp.lam0, *c = a.c + lp.x0, *xp0 = a.xp0 + lp.x0;
    double s0 = 0.0, s1 = 0.0, mr = -__builtin_inf(), c0 = 0.0, c1 = 0.0, mx = -__builtin_inf();
    for (i32 r = threadIdx.x; r < m; r += kBlock) {
        const i64 g = many_row(lp.eq0, lp.in0, lp.m_eq, r);
        const double ax = admm_dot<1>(a.aptr[g], a.aptr[g + 1], a.aidx, a.aval, x, AdmmLoadPlain());
        const double res = ax - b[r];
        s0 += res * res;
        s1 += lam[r] * res;
        const double ar = fabs(res);
        mr = ar > mr ? ar : mr;
    }
    for (i32 j = threadIdx.x; j < N; j += kBlock) {
        const double xj = x[j];
        const double dx = first ? xj - xp0[j] : 0.0;  // xp is x itself after the first multiplier step
        if (j < lp.n) c0 += c[j] * xj;                // the slack columns cost nothing
        c1 += dx * dx;
        mx = (-xj) > mx ? (-xj) : mx;
    }
    const double r0 = block_reduce<false>(s0, lds), r1 = block_reduce<false>(s1, lds), r2 = block_reduce<true>(mr, lds);
    const double r3 = block_reduce<false>(c0, lds), r4 = block_reduce<false>(c1, lds), r5 = block_reduce<true>(mx, lds);
    if (threadIdx.x == 0) {
        double *o = out + (i64)blockIdx.x * 3;
        o[0] = r3 + 0.5 * a.gamma_eq * r0 + 0.5 * a.gamma_ineq * r4 + r1;  // :124-132
        o[1] = r2;                                                          // :221
        o[2] = (r5 > 0.0) ? r5 : 0.0;                                       // :222
    }
}

}  // namespace slp

using namespace slp;

struct slp_admm_many {
    slp_admm *base = nullptr;  // owned: the composite's set-up; the index arrays of its A are local to the LPs once the set-up is done
    AdmmShared sh;
    i64 count = 0, n = 0, N = 0, m = 0, m_eq = 0;
    double gamma_eq = 2, gamma_ineq = 3;
    bool xp_is_x = false;      // false only before the first multiplier step (:98 vs :259)
    std::vector<AdmmmLp> lps;
    ManyGroup group[2];  // the LPs of each form
    DevBuf<i32> list[2];
    i64 cap = kManyMaxItersPerLaunch;  // SLP_ADMM_MANY_KMAX
    DevBuf<AdmmmLp> table;
    DevBuf<i64> gptr, lptr;
    DevBuf<i32> gidx, grows;
    DevBuf<double> gval, ginvd;
    DevBuf<double> b, q, c, lb, ub, xp0, x, y, lam, out;
    // stopping: off while tol_residual < 0.  The kernel without the test touches no record, so the whole iterations run while it is
    // off are counted here and added to every record when the test is armed (and when the state is read)
    DevBuf<AdmmmCtl> ctl;
    double tol_residual = -1.0, tol_step = 0.0;
    i64 check_every = 1, uncounted = 0;
    bool mid_iteration = false;  // between sweep_step and multiplier_step
    // compaction (slp_many_admm_set_compaction): the launches of an armed call run over the live list of each form
    ManyFormLists live;
    ~slp_admm_many() { if (base) slp_admm_destroy(base); }
};

namespace slp {

static AdmmmArgs admmm_args(const slp_admm_many *s, int g) {
    const CsrDev &A = s->sh.a->a, &At = s->sh.a->at;
    AdmmmArgs r;
    r.lps = s->table.p;
    r.list = s->list[g].p;
    r.tptr = At.ptr.p; r.tidx = At.idx.p; r.tval = At.val.p;
    r.aptr = A.ptr.p; r.aidx = A.idx.p; r.aval = A.val.p;
    r.gptr = s->gptr.p; r.gidx = s->gidx.p; r.gval = s->gval.p; r.ginvd = s->ginvd.p; r.grows = s->grows.p; r.lptr = s->lptr.p;
    r.b = s->b.p; r.q = s->q.p; r.c = s->c.p; r.lb = s->lb.p; r.ub = s->ub.p; r.xp0 = s->xp0.p;
    r.x = s->x.p; r.y = s->y.p; r.lam = s->lam.p;
    r.gamma_eq = s->gamma_eq; r.gamma_ineq = s->gamma_ineq;
    return r;
}

// one launch of form g over `wgs` workgroups.  LIVE (armed only): over the form's live list, built in front of it
template <bool LDS, bool LIVE>
static void admmm_launch(slp_admm_many *s, int g, AdmmmArgs a, i64 wgs, int it, int first, int stages, bool stop) {
    const ManyGroup &gr = s->group[g];
    const AdmmmStop sp = {s->ctl.p, s->tol_residual, s->tol_step, s->check_every};
    const dim3 grid((unsigned)wgs), block(gr.block);
    const size_t lds = LDS ? gr.lds_bytes : 0;
    const i32 *live_n = nullptr;
    if (LIVE) {
        many_form_list(s->live, s->group, g, s->table.p, s->ctl.p, s->count);
        a.list = s->live.ids[g].p;
        live_n = s->live.n[g].p;
    }
    if (stop) hipLaunchKernelGGL((k_admmm_iterate<LDS, true, LIVE>), grid, block, lds, ctx().stream, a, it, first, stages, sp, live_n);
    else hipLaunchKernelGGL((k_admmm_iterate<LDS, false, false>), grid, block, lds, ctx().stream, a, it, first, stages, sp, live_n);
}

// `k` times the stages, in launches of at most kmax iterations per form; with the stopping test when it is armed.  With compaction
// on an armed call reads the records back first (one download; it synchronises): per form its grid is the number of LPs live then,
// its cap that of so many workgroups (many_form_call), and every launch runs over the live list k_many_live builds in front of it
// -- an LP that stops in the call leaves the list at the next launch, the surplus workgroups return at its end.  A form without a
// live LP launches nothing.
static void admmm_run(slp_admm_many *s, i64 k, int stages) {
    if (k <= 0) return;
    const bool stop = s->tol_residual >= 0.0;
    if (!stop && (stages & 2)) s->uncounted += k;
    s->mid_iteration = !(stages & 2);
    const bool live = stop && s->live.on;
    ManyFormCall call = {};
    if (live) call = many_form_call(s->lps, many_read_ctl(s->ctl, s->count, s->uncounted).data(), s->group, ctx().num_cu, s->cap);
    for (int g = 0; g < 2; ++g) {
        const ManyGroup &gr = s->group[g];
        if (gr.ids.empty() || (live && call.live[g] == 0)) continue;
        const AdmmmArgs a = admmm_args(s, g);
        const i64 wgs = live ? call.live[g] : (i64)gr.ids.size(), cap = live ? call.cap[g] : gr.kmax;
        bool xp_is_x = s->xp_is_x;
        many_split(k, cap, [&](int it) {
            const int first = ((stages & 1) && !xp_is_x) ? 1 : 0;
            if (live) {
                if (g == 0) admmm_launch<true, true>(s, g, a, wgs, it, first, stages, stop);
                else admmm_launch<false, true>(s, g, a, wgs, it, first, stages, stop);
            } else {
                if (g == 0) admmm_launch<true, false>(s, g, a, wgs, it, first, stages, stop);
                else admmm_launch<false, false>(s, g, a, wgs, it, first, stages, stop);
            }
            s->live.launched[g] = wgs;
            s->live.cap[g] = cap;
            if (stages & 2) xp_is_x = true;  // :259
            return it;
        });
    }
    if (stages & 2) s->xp_is_x = true;
}

// the two environment switches and the form per LP -- from the shapes only; needs no device, nothing is allocated yet
static void admmm_forms(slp_admm_many *s) {
    const int force = many_form_switch("SLP_ADMM_MANY_FORM");
    s->cap = many_kmax_switch("SLP_ADMM_MANY_KMAX", s->cap);
    std::vector<i64> lds_doubles;
    for (const AdmmmLp &lp : s->lps) lds_doubles.push_back(2 * ((i64)lp.n + lp.m_in) + lp.m_eq + lp.m_in);
    const std::vector<i32> form =
        many_assign_forms(lds_doubles, kAdmmmLdsLimit, force, "slp_admm_many_create", "SLP_ADMM_MANY_FORM", "2 N + m", s->group);
    for (size_t k = 0; k < form.size(); ++k) s->lps[k].form = form[k];
}

// workgroup, LDS and launch cap per form, once the levels of every LP are known
static void admmm_plan(slp_admm_many *s) {
    for (int g = 0; g < 2; ++g) {
        ManyGroup &gr = s->group[g];
        if (gr.ids.empty()) continue;
        i64 want = 1, doubles = 0, passes = 1;
        for (i32 k : gr.ids) {
            const AdmmmLp &lp = s->lps[(size_t)k];
            const i64 N = (i64)lp.n + lp.m_in, m = (i64)lp.m_eq + lp.m_in;
            want = std::max<i64>(want, std::max<i64>(lp.widest, (std::max(N, m) + 3) / 4));
            doubles = std::max<i64>(doubles, 2 * N + m);
            passes = std::max<i64>(passes, (i64)lp.nlevels + 2);
        }
        gr.block = many_width(want, kAdmmmMaxBlock);
        gr.lds_bytes = g == 0 ? (size_t)doubles * sizeof(double) : 0;
        gr.passes = passes;
        gr.kmax = many_launch_cap(kManyUnitsPerLaunch, passes, (i64)gr.ids.size(), ctx().num_cu, s->cap);
    }
}

// M's level-ordered copy, LP by LP.  The host reads the row pointer, the row order and one flag per row of the composite's copy
// (index-sized arrays), gives every LP the levels of its own plan (the sink rule of gs_plan per LP) and the order (level, row);
// the entries move on the device.
static void admmm_regroup(slp_admm_many *s) {
    hipStream_t st = ctx().stream;
    const AdmmShared &sh = s->sh;
    const i64 N = s->N, n_all = s->n, count = s->count;
    std::vector<i32> rows((size_t)N);
    std::vector<i64> ptr((size_t)N + 1);
    std::vector<unsigned char> up((size_t)N);
    {
        DevBuf<unsigned char> dup((size_t)N);
        hipLaunchKernelGGL(k_admmm_coupled_up, dim3(grid_for(N, kBlock)), dim3(kBlock), 0, st, N, sh.gs_ptr, sh.gs_idx, sh.gs_rows, dup.p);
        SLP_HIP(hipGetLastError());
        SLP_HIP(hipMemcpyAsync(rows.data(), sh.gs_rows, (size_t)N * sizeof(i32), hipMemcpyDeviceToHost, st));
        SLP_HIP(hipMemcpyAsync(ptr.data(), sh.gs_ptr, ((size_t)N + 1) * sizeof(i64), hipMemcpyDeviceToHost, st));
        dup.download(up.data(), (size_t)N);
    }
    // the LP of a composite column: variables by col0, slacks by slack0
    std::vector<i64> vfirst((size_t)count), sfirst((size_t)count);
    for (i64 k = 0; k < count; ++k) { vfirst[(size_t)k] = s->lps[(size_t)k].col0; sfirst[(size_t)k] = s->lps[(size_t)k].slack0; }
    auto lp_of_col = [&](i64 j) {
        const std::vector<i64> &f = j < n_all ? vfirst : sfirst;
        // LPs without a slack share their slack start with the next LP: the last of those that begin at or before j has it
        return (i64)(std::upper_bound(f.begin(), f.end(), j) - f.begin()) - 1;
    };
    // per LP, in (composite level, row) order: the old position and the level of each of its rows
    std::vector<std::vector<i32>> pos((size_t)count), lev((size_t)count);
    std::vector<std::vector<unsigned char>> isup((size_t)count);
    for (i64 l = 0; l < sh.nlevels; ++l)
        for (i64 t = sh.lptr[(size_t)l]; t < sh.lptr[(size_t)l + 1]; ++t) {
            const i64 k = lp_of_col(rows[(size_t)t]);
            pos[(size_t)k].push_back((i32)t);
            lev[(size_t)k].push_back((i32)l);
            isup[(size_t)k].push_back(up[(size_t)t]);
        }
    const char *es = getenv("SLP_GS_SINKS");
    const bool sinks_on = !(es && es[0] == '0');
    std::vector<i32> src((size_t)N), lp_of((size_t)N);
    std::vector<i64> nptr((size_t)N + 1, 0), lptr;
    for (i64 k = 0; k < count; ++k) {
        AdmmmLp &lp = s->lps[(size_t)k];
        const size_t Nk = (size_t)lp.n + (size_t)lp.m_in;
        std::vector<i32> &lv = lev[(size_t)k];
        SLP_REQUIRE(lv.size() == Nk, "slp_admm_many_create: the composite's plan does not cover LP " + std::to_string(k));
        i32 maxlev = 0;
        for (i32 v : lv) maxlev = std::max(maxlev, v);
        // gs_plan's rule, on this LP alone: many rows that nothing waits for go to one level behind all others
        i64 sinks = 0;
        for (size_t r = 0; r < Nk; ++r) sinks += (!isup[(size_t)k][r] && lv[r] > 0) ? 1 : 0;
        if (sinks > kAdmmmSinks && sinks_on)
            for (size_t r = 0; r < Nk; ++r)
                if (!isup[(size_t)k][r] && lv[r] > 0) lv[r] = maxlev + 1;
        // renumber: the composite's levels this LP has no row in are gone
        std::vector<i32> remap((size_t)maxlev + 2, 0);
        for (i32 v : lv) remap[(size_t)v] = 1;
        i32 next_level = 0;
        for (size_t l = 0; l < remap.size(); ++l) remap[l] = remap[l] ? next_level++ : -1;
        lp.nlevels = next_level;
        lp.lptr0 = (i64)lptr.size();
        std::vector<i64> start((size_t)next_level + 1, 0);
        for (i32 &v : lv) { v = remap[(size_t)v]; start[(size_t)v + 1]++; }
        i64 widest = 0;
        for (i32 l = 0; l < next_level; ++l) { widest = std::max(widest, start[(size_t)l + 1]); start[(size_t)l + 1] += start[(size_t)l]; }
        lp.widest = (i32)widest;
        lptr.insert(lptr.end(), start.begin(), start.end());
        // stable by level: the rows of a level stay in increasing row order
        for (size_t r = 0; r < Nk; ++r) {
            const i64 p = lp.x0 + start[(size_t)lv[r]]++;
            src[(size_t)p] = pos[(size_t)k][r];
            lp_of[(size_t)p] = (i32)k;
        }
    }
    for (i64 p = 0; p < N; ++p) nptr[(size_t)p + 1] = nptr[(size_t)p] + (ptr[(size_t)src[(size_t)p] + 1] - ptr[(size_t)src[(size_t)p]]);
    const i64 nnz = nptr[(size_t)N];
    s->table.upload(s->lps.data(), (size_t)count);
    s->lptr.upload(lptr.data(), lptr.size());
    s->gptr.upload(nptr.data(), (size_t)N + 1);
    s->gidx.alloc((size_t)nnz); s->gval.alloc((size_t)nnz); s->ginvd.alloc((size_t)N); s->grows.alloc((size_t)N);
    DevBuf<i32> dsrc, dlp;
    dsrc.upload(src.data(), (size_t)N);
    dlp.upload(lp_of.data(), (size_t)N);
    hipLaunchKernelGGL(k_admmm_regroup, dim3(grid_for(N, kBlock)), dim3(kBlock), 0, st, N, s->table.p, dlp.p, dsrc.p, sh.gs_ptr, sh.gs_idx, sh.gs_val,
                       sh.gs_invd, sh.gs_rows, n_all, s->gptr.p, s->gidx.p, s->gval.p, s->ginvd.p, s->grows.p);
    SLP_HIP(hipGetLastError());
    SLP_HIP(hipStreamSynchronize(st));  // dsrc, dlp go away
}

}  // namespace slp

extern "C" {

int64_t slp_admm_many_lds_limit(void) { return kAdmmmLdsLimit; }

slp_admm_many *slp_admm_many_create(int64_t count, const int64_t *n, const int64_t *m_eq, const int64_t *m_ineq,
                                    const int64_t *eq_indptr, const int32_t *eq_indices, const double *eq_data, const double *b_eq,
                                    const int64_t *in_indptr, const int32_t *in_indices, const double *in_data, const double *b_lower,
                                    const double *b_upper, const double *c, const double *lb, const double *ub, const double *x0,
                                    double gamma_eq, double gamma_ineq, int use_preconditioning) {
    SLP_API_PTR({
        SLP_REQUIRE(count >= 1, "slp_admm_many_create: count must be at least 1");
        SLP_REQUIRE(n && m_eq && m_ineq && c && lb && ub, "slp_admm_many_create: NULL argument");
        SLP_REQUIRE(in_indptr, "slp_admm_many_create: the inequality block is required (the reference's standard form is undefined "
                               "without it, tools.py:92)");
        // everything below up to the memory check reads the host arrays only: nothing is allocated before the list is known to be
        // well formed and to fit
        auto s = std::unique_ptr<slp_admm_many>(new slp_admm_many());
        s->count = count; s->gamma_eq = gamma_eq; s->gamma_ineq = gamma_ineq;
        s->lps.resize((size_t)count);
        i64 nn = 0, Me = 0, Mi = 0;
        for (i64 k = 0; k < count; ++k) {
            SLP_REQUIRE(n[k] >= 1 && m_eq[k] >= 0 && m_ineq[k] >= 0, "slp_admm_many_create: every LP needs at least one variable");
            AdmmmLp &lp = s->lps[(size_t)k];
            lp.col0 = nn; lp.slack0 = Mi; lp.eq0 = Me; lp.in0 = Mi;  // slack0, in0: completed below, once n and m_eq are summed
            lp.x0 = nn + Mi; lp.lam0 = Me + Mi; lp.lptr0 = 0;
            nn += n[k]; Me += m_eq[k]; Mi += m_ineq[k];
            SLP_REQUIRE(nn + Mi < ((i64)1 << 31) && Me + Mi < ((i64)1 << 31),
                        "slp_admm_many_create: the list has 2^31 or more variables + slacks or rows");
            lp.n = (i32)n[k]; lp.m_eq = (i32)m_eq[k]; lp.m_in = (i32)m_ineq[k];
            lp.nlevels = 0; lp.widest = 0; lp.form = 0;
        }
        for (AdmmmLp &lp : s->lps) { lp.slack0 += nn; lp.in0 += Me; }
        const i64 N = nn + Mi, M = Me + Mi;
        s->n = nn; s->N = N; s->m = M; s->m_eq = Me;
        SLP_REQUIRE(Me == 0 || (eq_indptr && b_eq), "slp_admm_many_create: NULL equality block");
        auto check_block = [&](const char *what, const int64_t *indptr, const int32_t *indices, const double *data, i64 rows, bool ineq) {
            std::vector<ManyRows> of_lp;
            for (i64 k = 0; k < count; ++k) {
                const AdmmmLp &lp = s->lps[(size_t)k];
                const i64 r0 = ineq ? lp.in0 - Me : lp.eq0;
                of_lp.push_back({k, r0, r0 + (ineq ? lp.m_in : lp.m_eq), lp.col0, lp.col0 + lp.n});
            }
            const std::string block = std::string("the ") + what + " block";
            many_check_block({"slp_admm_many_create", "the row pointer of " + block, "decreases", block + " of ", false}, indptr, indices,
                             indices && data, rows, of_lp);
        };
        if (Me) check_block("equality", eq_indptr, eq_indices, eq_data, Me, false);
        check_block("inequality", in_indptr, in_indices, in_data, Mi, true);
        admmm_forms(s.get());
        {
            // both copies of A with the scratch of the chain, M twice (the plan's copy and the regrouped one) with the lane records
            // of the SpGEMM (at most the sum of squared row lengths entries), thirteen vectors over the columns and four over the rows
            double nnz_a = (double)in_indptr[Mi] + (double)Mi + (Me ? (double)eq_indptr[Me] : 0.0), sq = 0.0;
            for (i64 i = 0; i < Mi; ++i) { const double l = (double)(in_indptr[i + 1] - in_indptr[i]) + 1.0; sq += l * l; }
            for (i64 i = 0; i < Me; ++i) { const double l = (double)(eq_indptr[i + 1] - eq_indptr[i]); sq += l * l; }
            many_require_memory("slp_admm_many_create", count,
                                64.0 * nnz_a + 52.0 * (sq + (double)N) + 8.0 * (13.0 * (double)N + 4.0 * (double)M) + 16.0 * 8.0 * (double)(N + M) +
                                    (double)count * (double)(sizeof(AdmmmLp) + sizeof(AdmmmCtl) + sizeof(i32) + 3 * sizeof(double)));
        }
        hipStream_t st = ctx().stream;
        // the whole chain once, on the composite (its x0 = [x0; A_ineq x0] block by block: the scaled block is block-diagonal too)
        s->base = admm_create_lp(nn, Me, Me ? eq_indptr : nullptr, eq_indices, eq_data, b_eq, Mi, in_indptr, in_indices, in_data, b_lower, b_upper,
                                 c, lb, ub, x0, gamma_eq, gamma_ineq, use_preconditioning, SLP_ORDER_SEQUENTIAL, nullptr, true, true);
        admm_shared(s->base, &s->sh);
        require_csr(s->sh.a, "slp_admm_many_create");
        admmm_regroup(s.get());  // uploads the table
        admmm_plan(s.get());
        const CsrDev &A = s->sh.a->a, &At = s->sh.a->at;
        const dim3 per_lp((unsigned)count);
        hipLaunchKernelGGL(k_admmm_localise, per_lp, dim3(kBlock), 0, st, s->table.p, A.ptr.p, A.idx.p, At.ptr.p, At.idx.p, nn, Me);
        SLP_HIP(hipGetLastError());
        many_upload_lists(s->group, s->list);
        for (const void *kernel : {reinterpret_cast<const void *>(k_admmm_iterate<true, false, false>),
                                   reinterpret_cast<const void *>(k_admmm_iterate<true, true, false>),
                                   reinterpret_cast<const void *>(k_admmm_iterate<true, true, true>)})
            many_lds_opt_in(kernel, s->group[0].lds_bytes, kAdmmmLdsLimit * sizeof(double));
        s->b.alloc((size_t)M); s->lam.alloc((size_t)M); s->lam.zero();
        for (DevBuf<double> *v : {&s->q, &s->c, &s->lb, &s->ub, &s->xp0, &s->x, &s->y}) v->alloc((size_t)N);
        s->y.zero();
        const std::pair<const double *, double *> cols[] = {{s->sh.q, s->q.p},   {s->sh.c, s->c.p},     {s->sh.lb, s->lb.p},
                                                            {s->sh.ub, s->ub.p}, {s->sh.xp0, s->xp0.p}, {s->sh.x0, s->x.p}};
        for (const auto &v : cols) hipLaunchKernelGGL(k_admmm_gather_cols, per_lp, dim3(kBlock), 0, st, s->table.p, v.first, v.second);
        hipLaunchKernelGGL(k_admmm_gather_rows, per_lp, dim3(kBlock), 0, st, s->table.p, s->sh.b, s->b.p);
        SLP_HIP(hipGetLastError());
        s->out.alloc((size_t)3 * (size_t)count);
        std::vector<AdmmmCtl> ctl((size_t)count, AdmmmCtl{{0, 0, 0, 0}, __builtin_inf(), __builtin_inf(), 0.0});
        s->ctl.upload(ctl.data(), ctl.size());
        SLP_HIP(hipStreamSynchronize(st));
        return s.release();
    })
}

void slp_admm_many_destroy(slp_admm_many *s) { delete s; }

int slp_admm_many_iterate(slp_admm_many *s, int64_t k) {
    SLP_API_INT({ SLP_REQUIRE(s && k >= 0, "slp_admm_many_iterate: bad arguments"); admmm_run(s, k, 3); })
}

int slp_admm_many_sweep_step(slp_admm_many *s) { SLP_API_INT({ SLP_REQUIRE(s, "NULL handle"); admmm_run(s, 1, 1); }) }

int slp_admm_many_multiplier_step(slp_admm_many *s) { SLP_API_INT({ SLP_REQUIRE(s, "NULL handle"); admmm_run(s, 1, 2); }) }

int slp_admm_many_report(slp_admm_many *s, double *out) {
    SLP_API_INT({
        SLP_REQUIRE(s && out, "slp_admm_many_report: NULL argument");
        hipLaunchKernelGGL(k_admmm_report, dim3((unsigned)s->count), dim3(kBlock), 0, ctx().stream, admmm_args(s, 0), s->xp_is_x ? 0 : 1, s->out.p);
        SLP_HIP(hipGetLastError());
        s->out.download(out, (size_t)3 * (size_t)s->count);
    })
}

int slp_many_admm_set_stop(slp_admm_many *s, double tol_residual, double tol_step, int64_t check_every) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_admm_set_stop: NULL handle");
        SLP_REQUIRE(tol_residual < 0.0 || (std::isfinite(tol_residual) && std::isfinite(tol_step) && tol_step >= 0.0 && check_every >= 1),
                    "slp_many_admm_set_stop: tol_residual and tol_step must be finite and >= 0 with check_every >= 1 (tol_residual < 0 turns "
                    "the test off)");
        SLP_REQUIRE(!s->mid_iteration, "slp_many_admm_set_stop: called between sweep_step and multiplier_step (whole iterations only)");
        many_rearm(s->ctl, s->count, &s->uncounted);
        s->tol_residual = tol_residual < 0.0 ? -1.0 : tol_residual;
        if (tol_residual >= 0.0) {
            s->tol_step = tol_step;
            s->check_every = check_every;
        }
    })
}

int slp_many_admm_stop_state(slp_admm_many *s, int64_t *iterations, int32_t *stopped, double *residual, double *step) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_admm_stop_state: NULL handle");
        const std::vector<AdmmmCtl> h = many_read_ctl(s->ctl, s->count, s->uncounted);
        for (size_t k = 0; k < h.size(); ++k) {
            many_state_head(h[k], k, iterations, stopped);
            if (residual) residual[k] = h[k].residual;
            if (step) step[k] = h[k].step;
        }
    })
}

int slp_many_admm_set_compaction(slp_admm_many *s, int on) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_admm_set_compaction: NULL handle");
        SLP_REQUIRE(on == 0 || on == 1, "slp_many_admm_set_compaction: on must be 0 or 1");
        if (on) many_form_alloc(s->live, s->group);
        s->live.on = on != 0;
    })
}

int slp_many_admm_live_state(slp_admm_many *s, int64_t live[2], int32_t *order, int64_t launched[2], int64_t cap[2]) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_admm_live_state: NULL handle");
        many_form_state("slp_many_admm_live_state", s->live, s->group, s->table.p, s->ctl.p, s->count, live, order, launched, cap);
    })
}

int slp_admm_many_get_x(slp_admm_many *s, double *x, int full) {
    SLP_API_INT({
        SLP_REQUIRE(s && x, "slp_admm_many_get_x: NULL argument");
        if (full) {
            s->x.download(x, (size_t)s->N);
        } else {  // the first n_k entries of every LP (:268)
            std::vector<double> h((size_t)s->N);
            s->x.download(h.data(), (size_t)s->N);
            for (const AdmmmLp &lp : s->lps) std::copy(h.begin() + lp.x0, h.begin() + lp.x0 + lp.n, x + lp.col0);
        }
    })
}

int slp_admm_many_get_lambda(slp_admm_many *s, double *lam) {
    SLP_API_INT({ SLP_REQUIRE(s && lam, "NULL argument"); s->lam.download(lam, (size_t)s->m); })
}

int64_t slp_admm_many_num_levels(const slp_admm_many *s, int64_t k) { return (s && k >= 0 && k < s->count) ? s->lps[(size_t)k].nlevels : -1; }

int slp_admm_many_form(const slp_admm_many *s, int64_t k) { return (s && k >= 0 && k < s->count) ? s->lps[(size_t)k].form : -1; }

int64_t slp_admm_many_kmax(const slp_admm_many *s, int form) { return (s && (form == 0 || form == 1)) ? (s->group[form].ids.empty() ? 0 : s->group[form].kmax) : -1; }

int slp_admm_many_bench(slp_admm_many *s, int64_t k, double *ms) {
    SLP_API_INT({
        SLP_REQUIRE(s && k > 0 && ms, "slp_admm_many_bench: bad arguments");
        Context &c = ctx();
        float f = 0.f;
        SLP_HIP(hipEventRecord(c.ev0, c.stream));
        admmm_run(s, k, 3);
        SLP_HIP(hipEventRecord(c.ev1, c.stream));
        SLP_HIP(hipEventSynchronize(c.ev1));
        SLP_HIP(hipEventElapsedTime(&f, c.ev0, c.ev1));
        *ms = (double)f / (double)k;
    })
}

}  // extern "C"
