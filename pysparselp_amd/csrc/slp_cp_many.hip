// slp_cp_many.hip -- Chambolle-Pock on a SET of LPs whose constraint matrices differ: one workgroup per LP, whole iterations
// inside one launch.  No counterpart in the reference (single-threaded numpy: N solves are N calls of chambolle_pock_ppd,
// ChambollePockPPD.py:36-346, each of them two launches per iteration here and bound by launch latency when the LP is small).
// An iteration of the method has no global scalar -- no dot product, no step size beyond the per-row Sigma and the per-column T --
// so it is two sparse walks separated by a barrier, and N independent LPs are N independent workgroups:
//   primal half : a lane walks its column of K^T, d = (c + se) + si, x+ = clip(x - T d), z = (1+theta) x+ - theta x   [:198-228]
//   barrier
//   dual half   : a lane walks its row of K, y += Sigma (K z - b), inequality rows clamped at 0                        [:231-240,:333-342]
//   barrier
// with the device functions of slp_cp_shared.h: every LP is bit for bit the iterate of slp_cp in SLP_ORDER_SEQUENTIAL on that LP.
//
// Layout.  The K_k = [A_eq,k; A_ineq,k] form ONE block-diagonal CSR: the columns of LP k are offset by sum_{l<k} n_l; the rows are
// all equality rows (LP 0, LP 1, ...) followed by all inequality rows, so that "row < m_eq" with the global m_eq = sum m_eq,k
// tells the two kinds apart and the set-up of the single solver (build_transpose: rows increasing inside a column;
// cp_preconditioners_csr: per-column and per-row sums) gives every LP the entry order and the T, Sigma of its own set-up.  After
// that set-up the index arrays of both orientations are rewritten IN PLACE to indices local to their LP (column - col0; row
// - eq0, or m_eq,k + row - in0): both forms of the kernel then address an LP's vectors from their base, in LDS or in global memory.
// x, z, x4, c, lb, ub, T are concatenated LP by LP; y is kept LP by LP as [y_eq,k; y_ineq,k]; b and Sigma in the row order of K.
// CpmLp, one per LP, holds its column range and its two row ranges.
//
// Forms, workgroup width and launch cap: slp_many_plan.h (switches SLP_CP_MANY_FORM, SLP_CP_MANY_KMAX).  Here the lds form holds
// x, z, y (2 n + m <= kCpmLdsLimit doubles; the global form as k_admmb_tile, k_gs_sweep_one_block); c, T, lb, ub, b, Sigma are read
// from global memory in both.  A launch wants max_k max(n_k, m_k) lanes, and a pass is the workgroup once over its columns or rows.
// No atomics between workgroups, no spin waits, no grid barrier: a workgroup never waits for another.
//
// Report, per LP, one workgroup of 256 lanes on the written-back state: lane t takes rows (columns) t, t + 256, ... in increasing
// order -- per row the three chains K x, K x4, K z of one walk -- then block_reduce: a fixed order, a function of the shapes only.
// The maxima are exact.  x4 is written by the primal half of a reporting iteration.
//
// One text per piece.  cpm_open (the view of an LP, with the LDS fill) and cpm_close (the write-back), cpm_direction (d_j),
// cpm_primal_half<STEP> and cpm_dual_half<STEP> (a half without its barrier; STEP: the lane's nan-max of what it changed) are
// device functions used by every iterate kernel below.  The stopping protocol -- the head of the record (ManyCtl), entering from
// it, a wave's slot, lane 0's fold, the decision slot with its barrier -- is slp_many.h's, shared with slp_admm_many.hip; the
// scalar arithmetic of the certificate is slp_cp_gap.h's, shared with slp_cp_batch.hip and compiled for the host by a test.
//
// Stopping (slp_many_cp_set_stop; off after create).  CpmCtl, one per LP in device memory: iterations completed, the stopped flag,
// the stopping iteration and the last evaluated step.  Iterations of an LP count from 1 over its whole life; at the end of an
// iteration t with t % check_every == 0 the LP stops iff step = max(max_j |x2_j - x_j|, max_r |y_r+ - y_r|) <= tol, the differences
// those of iteration t alone (a lane holds both values of what it updates) and the maximum NaN-propagating as np.max: exact in any
// order, so the decision is that of a CPU restatement.  The test is the template parameter STOP of k_cpm_iterate: STOP = false is
// the kernel without it -- no extra barrier, no word of the control record read or written (the host counts the iterations).
// With STOP a wave reduces its lanes' maxima by shuffles into one LDS slot per wave and half before the barrier that ends the
// half; after the dual half's barrier lane 0 folds the slots, writes the record and ONE LDS slot with the decision, and one more
// barrier later every lane reads that slot: the break is uniform, and so is every barrier.  A stopped LP's workgroup returns before
// its first barrier (the flag was written by an earlier launch: the same for every lane) and its x, z, y are never written again;
// in the launch in which it stops it leaves the loop and, in the lds form, writes its iterates back.  Between primal_step and
// dual_step the reduced dx waits in the record.  The count of an LP is read from the record at the start of a launch, so the
// stopping iteration does not depend on how a run is split into launches.
//
// Stopping on a certified duality gap (slp_many_cpgap_set_stop; arming one test disarms the other).  y is dual feasible for a
// box-bounded LP by construction (free equality multipliers, clamped inequality multipliers), so with d = c + K^T y_t -- the bits
// the next primal half computes -- bound = sum_j [d_j != 0 ? min(d_j lb_j, d_j ub_j) : 0] - sum_r [y_r != 0 ? y_r b_r : 0] is a
// lower bound on the LP's value (the reference's energy2, :262-266, evaluated there at reports only); primal = sum_j c_j x_t,j;
// violation = max(max_{r < m_eq} |(K x_t)_r - b_r|, max_{r >= m_eq} ((K x_t)_r - b_r), 0) with K x_t a single-accumulator chain
// in storage order and the maximum NaN-propagating: exact in any order.  At the end of an iteration t with t % check_every == 0 the LP
// stops iff violation <= tol_feas and |primal - bound| <= tol_gap (1 + |primal| + |bound|) with a finite left-hand side (inf <=
// tol_gap * inf holds in IEEE arithmetic; a bound of -inf must not stop).  k_cpm_iterate_gap is the third kind of k_cpm_iterate.  An
// iteration that is no check is cpm_primal_half<false> and cpm_dual_half<false>, the halves of STOP = false, plus two scalar
// counters.  A check iteration has a dual loop of its own -- K x beside K z in one row walk (cp_row_sums2), per lane
// sum y_r b_r over its rows in increasing order and the nan-max of the violation -- then, behind the dual half's barrier, one pass over
// the columns (d_j, its term of the bound, c_j x_j).  A wave reduces its lanes by shuffles in a fixed order (many_wave_reduce:
// two quantities side by side) into one LDS slot per quantity; behind one more barrier lane 0 folds each quantity over the waves in increasing
// order (many_fold: one loop, four chains), writes the record CpmGap (primal, bound, violation: +inf, -inf, +inf before the first check) and ONE decision slot, and a
// last barrier later every lane reads it.  The two sums are in that fixed order, a function of the shapes only.  The head of
// CpmCtl is shared with the step test; nothing waits in a record between primal_step and dual_step.
//
// Compaction (slp_many_cp_set_compaction, include/slp_hip_ext_many_live.h; off after create): the template parameter LIVE of the
// two armed kernels.  Without it a stopped LP keeps its workgroup index, the launch its full grid and its cap.  With compaction on
// and a test armed, cpm_run reads the records back at the start of a call (one download; it synchronises), and per form every
// launch of the call is preceded by k_many_live<ManyFormLive<CpmLp, CpmCtl>> (slp_many.h: the LPs of that form that are not
// stopped, in increasing order, and their count) and is <., ., true> over as many workgroups as LPs of the form were live when
// the call began, held to the cap of that many workgroups (many_form_call, slp_many_plan.h): a.list is the live list, a workgroup
// at or past *live_n returns before anything else.  A form without a live LP launches nothing.  An LP's iterations read and write
// its own data only, so which workgroup runs them changes no bit.  <., ., false> never looks at live_n: the kernels above.
#include <algorithm>
#include <cmath>
#include <memory>
#include <type_traits>

#include "slp_cp_shared.h"
#include "slp_kernels.h"
#include "slp_many.h"
#include "../../include/slp_hip_ext_many_live.h"

namespace slp {

// slp_cp.hip: T and Sigma by the CSR walks of the single-instance set-up
void cp_preconditioners_csr(slp_matrix *k, i64 m_eq, double alpha, double *t, double *sigma);

constexpr int kCpmMaxBlock = 1024;
// doubles of x, z, y an LP may hold in LDS: 160 000 of the compute unit's 163 840 bytes; the rest stays free for a kernel's static
// scratch (block_reduce: 32 bytes)
constexpr i64 kCpmLdsLimit = 20000;

struct CpmLp {
    i64 col0;      // first column: x, z, x4, c, lb, ub, T; rows of K^T
    i64 eq0, in0;  // first equality row, first inequality row in K: b, Sigma, row pointers
    i64 y0;        // where [y_eq; y_ineq] lie in y
    i32 n, m_eq, m_in;
    i32 form;      // 0 lds, 1 global
};

// the index arrays of both orientations, global -> local to the LP; one workgroup per LP
__global__ __launch_bounds__(kBlock) void k_cpm_localise(const CpmLp *__restrict__ lps, const i64 *__restrict__ ptr, i32 *__restrict__ idx,
                                                         const i64 *__restrict__ tptr, i32 *__restrict__ tidx, i64 m_eq_all) {
    const CpmLp lp = lps[blockIdx.x];
    const i32 m = lp.m_eq + lp.m_in;
    for (i32 r = threadIdx.x; r < m; r += kBlock) {
        const i64 g = many_row(lp.eq0, lp.in0, lp.m_eq, r);
        for (i64 q = ptr[g]; q < ptr[g + 1]; ++q) idx[q] = (i32)(idx[q] - lp.col0);
    }
    for (i32 j = threadIdx.x; j < lp.n; j += kBlock)
        for (i64 q = tptr[lp.col0 + j]; q < tptr[lp.col0 + j + 1]; ++q) {
            const i64 g = tidx[q];
            tidx[q] = (i32)(g < m_eq_all ? g - lp.eq0 : lp.m_eq + (g - lp.in0));
        }
}

// per LP, in device memory: the head of slp_many.h and what the step test evaluates
struct CpmCtl : ManyCtl {
    double step;  // the last evaluated step, +inf before the first test
    double dx;    // the primal half's maximum of a check iteration, carried from primal_step to dual_step
};

struct CpmStop {
    CpmCtl *ctl;
    double tol;
    i64 check_every;
};

constexpr int kCpmWaves = kCpmMaxBlock / kWave;

struct CpmArgs {
    const CpmLp *lps;
    const i32 *list;  // the LPs of this launch
    const i64 *ptr, *tptr;
    const i32 *idx, *tidx;  // local indices
    const double *val, *tval, *c, *t, *lb, *ub, *b, *sigma;
    double *x, *z, *y, *x4;
    double one_plus_theta, theta;
};

// What the lanes of an LP's workgroup work on: where its iterates lie (xs, zs, ys: LDS in the lds form, else the global
// xg, zg, yg) and its columns' data.
struct CpmView {
    CpmLp lp;
    i32 n, m, W, tid;
    double *xg, *zg, *yg, *xs, *zs, *ys;
    const double *c, *t, *lb, *ub;
    const i64 *tptr;
};

// the view of LP `id`; LDS: x, z, y are copied into `lds`, and a barrier follows
template <bool LDS>
__device__ __forceinline__ CpmView cpm_open(const CpmArgs &a, i32 id, double *lds) {
    CpmView v;
    v.lp = a.lps[id];
    v.n = v.lp.n, v.m = v.lp.m_eq + v.lp.m_in, v.W = (i32)blockDim.x, v.tid = (i32)threadIdx.x;
    v.xg = a.x + v.lp.col0, v.zg = a.z + v.lp.col0, v.yg = a.y + v.lp.y0;
    v.xs = v.xg, v.zs = v.zg, v.ys = v.yg;
    if (LDS) {
        v.xs = lds;
        v.zs = v.xs + v.n;
        v.ys = v.zs + v.n;
        for (i32 j = v.tid; j < v.n; j += v.W) { v.xs[j] = v.xg[j]; v.zs[j] = v.zg[j]; }
        for (i32 r = v.tid; r < v.m; r += v.W) v.ys[r] = v.yg[r];
        __syncthreads();
    }
    v.c = a.c + v.lp.col0, v.t = a.t + v.lp.col0, v.lb = a.lb + v.lp.col0, v.ub = a.ub + v.lp.col0;
    v.tptr = a.tptr + v.lp.col0;
    return v;
}

// the lds form writes its iterates back, at the end of a launch
template <bool LDS>
__device__ __forceinline__ void cpm_close(const CpmView &v) {
    if (LDS) {
        for (i32 j = v.tid; j < v.n; j += v.W) { v.xg[j] = v.xs[j]; v.zg[j] = v.zs[j]; }
        for (i32 r = v.tid; r < v.m; r += v.W) v.yg[r] = v.ys[r];
    }
}

// d_j = c_j + (K^T y)_j of column j, the bits the primal half computes
template <class LD>
__device__ __forceinline__ double cpm_direction(const CpmArgs &a, const CpmView &v, LD ld, i32 j) {
    double se, si;
    cp_column_sums(v.tptr[j], v.tptr[j + 1], a.tidx, a.tval, v.ys, 1, v.lp.m_eq, ld, &se, &si);
    return cp_direction(v.c[j], se, si, v.lp.m_eq > 0, v.lp.m_in > 0);
}

// The primal half without its barrier: a lane walks its columns; store: it also writes x4 (:260-261).  STEP: returns the lane's
// nan-max of |x+ - x| over its columns, 0.0 without it.
template <bool STEP, class LD>
__device__ __forceinline__ double cpm_primal_half(const CpmArgs &a, const CpmView &v, LD ld, int store) {
    double dx = 0.0;
    for (i32 j = v.tid; j < v.n; j += v.W) {
        const double d = cpm_direction(a, v, ld, j);
        const double xo = ld(v.xs + j), l = v.lb[j], u = v.ub[j];
        double x2, zn;
        cp_primal_point(d, xo, v.t[j], l, u, a.one_plus_theta, a.theta, &x2, &zn);
        v.zs[j] = zn;
        v.xs[j] = x2;
        if (store) a.x4[v.lp.col0 + j] = (d < 0.0) ? u : l;
        if (STEP) dx = nan_max(dx, fabs(x2 - xo));
    }
    return dx;
}

// The dual half without its barrier: a lane walks its rows.  STEP: returns the lane's nan-max of |y+ - y|, 0.0 without it.
template <bool STEP, class LD>
__device__ __forceinline__ double cpm_dual_half(const CpmArgs &a, const CpmView &v, LD ld) {
    double dy = 0.0;
    for (i32 r = v.tid; r < v.m; r += v.W) {
        const i64 g = many_row(v.lp.eq0, v.lp.in0, v.lp.m_eq, r);
        const double kz = cp_row_sum(a.ptr[g], a.ptr[g + 1], a.idx, a.val, v.zs, 1, ld);
        const double yo = ld(v.ys + r), yn = cp_dual_point(kz, a.b[g], yo, a.sigma[g], r >= v.lp.m_eq);
        v.ys[r] = yn;
        if (STEP) dy = nan_max(dy, fabs(yn - yo));
    }
    return dy;
}

// `iters` times the stages of one LP (bit 0 primal half, bit 1 dual half); store: the primal half also writes x4.
// STOP: the step test of the header comment, by the protocol of slp_many.h; `sp` is not looked at without it.
// LIVE (with STOP only): a.list is the form's live list, which k_many_live wrote in front of this launch, and *live_n its length; a
// workgroup at or past it returns before anything else (*live_n is the same for every lane).  `live_n` is not looked at without it.
template <bool LDS, bool STOP, bool LIVE>
__global__ __launch_bounds__(kCpmMaxBlock) void k_cpm_iterate(CpmArgs a, int iters, int stages, int store, CpmStop sp, const i32 *live_n) {
    static_assert(STOP || !LIVE, "an unarmed state has no stopped LP: no live variant");
    extern __shared__ __attribute__((aligned(16))) double cpm_lds[];
    __shared__ double cpm_red[STOP ? 2 * kCpmWaves + 1 : 1];  // per wave the maxima of the two halves, then the decision
    using LD = typename std::conditional<LDS, CpLoadPlain, CpLoadWorkgroup>::type;
    const LD ld;
    if (LIVE && blockIdx.x >= (unsigned)*live_n) return;
    const i32 id = a.list[blockIdx.x];
    i64 done = 0, until = 0;
    if (STOP && !many_enter(sp.ctl + id, sp.check_every, &done, &until)) return;
    const CpmView v = cpm_open<LDS>(a, id, cpm_lds);
    for (int it = 0; it < iters; ++it) {
        const bool check = STOP && until == 1;  // uniform: a function of the record and of `it`
        if (stages & 1) {
            double dx = cpm_primal_half<STOP>(a, v, ld, store);
            if (check) many_post<1, 1>(cpm_red, kCpmWaves, v.tid, &dx);
            __syncthreads();  // same compute unit: the stores of this half are visible to the next one
        }
        if (STOP && !(stages & 2)) {  // primal_step: the reduced dx waits in the record for dual_step
            if (check && v.tid == 0) {
                double dx;
                many_fold<1, 1>(cpm_red, kCpmWaves, v.W, &dx);
                sp.ctl[id].dx = dx;
            }
            continue;
        }
        if (stages & 2) {
            double dy = cpm_dual_half<STOP>(a, v, ld);
            if (check) many_post<1, 1>(cpm_red + kCpmWaves, kCpmWaves, v.tid, &dy);
            __syncthreads();
        }
        if (STOP) {  // here an iteration is complete
            ++done;
            if (!check) {
                --until;
                continue;
            }
            until = sp.check_every;
            if (v.tid == 0) {
                CpmCtl *ctl = sp.ctl + id;
                // dx, dy.  dual_step: dx waited in the record.  It is named up front and the compiler sinks the load into that
                // case; read inside the `else` the lds form takes 49 VGPRs for the parent's 48
                double f[2] = {ctl->dx, 0.0};
                if (stages & 1) many_fold<2, 3>(cpm_red, kCpmWaves, v.W, f);
                else many_fold<1, 1>(cpm_red + kCpmWaves, kCpmWaves, v.W, f + 1);
                const double step = nan_max(f[0], f[1]);
                ctl->step = step;
                many_decide(ctl, done, step <= sp.tol, cpm_red + 2 * kCpmWaves);  // false for a NaN
            }
            if (many_decided(cpm_red + 2 * kCpmWaves)) break;
        }
    }
    if (STOP && (stages & 2) && v.tid == 0) sp.ctl[id].done = done;
    cpm_close<LDS>(v);
}

// per LP, beside CpmCtl: the numbers of the last evaluated certificate (+inf, -inf, +inf before the first); written by lane 0 of
// the LP's workgroup in a check iteration of k_cpm_iterate_gap only
struct CpmGap {
    double primal, bound, violation;
};

struct CpmGapStop {
    CpmCtl *ctl;  // the head is shared with the step test; step and dx are not touched
    CpmGap *rec;
    double tol_gap, tol_feas;
    i64 check_every;
};

// k_cpm_iterate with the duality-gap certificate (slp_cp_gap.h) as the per-LP stopping test (header comment).  An iteration that
// is no check is the two halves above plus two scalar counters; a check iteration has its own dual loop and the certificate's
// pass over the columns.  Every branch around a barrier is on `stages`, `until`, the record or the decision slot: uniform.
// LIVE: as in k_cpm_iterate.
template <bool LDS, bool LIVE>
__global__ __launch_bounds__(kCpmMaxBlock) void k_cpm_iterate_gap(CpmArgs a, int iters, int stages, int store, CpmGapStop sp, const i32 *live_n) {
    extern __shared__ __attribute__((aligned(16))) double cpm_lds[];
    __shared__ double cpm_red[4 * kCpmWaves + 1];  // per wave: sum y b, violation, c x, the bound's column terms; then the decision
    using LD = typename std::conditional<LDS, CpLoadPlain, CpLoadWorkgroup>::type;
    const LD ld;
    if (LIVE && blockIdx.x >= (unsigned)*live_n) return;
    const i32 id = a.list[blockIdx.x];
    i64 done, until;
    if (!many_enter(sp.ctl + id, sp.check_every, &done, &until)) return;
    const CpmView v = cpm_open<LDS>(a, id, cpm_lds);
    for (int it = 0; it < iters; ++it) {
        if (stages & 1) {
            cpm_primal_half<false>(a, v, ld, store);
            __syncthreads();  // same compute unit: the stores of this half are visible to the next one
        }
        if (!(stages & 2)) continue;  // primal_step: the certificate needs nothing of this half but x itself
        if (until != 1) {             // no check
            cpm_dual_half<false>(a, v, ld);
            __syncthreads();
            ++done;
            --until;
            continue;
        }
        // a check iteration: the dual half with K x beside K z, then the certificate pass over the columns
        double rows[2] = {0.0, 0.0};  // sum y b, violation
        for (i32 r = v.tid; r < v.m; r += v.W) {
            const i64 g = many_row(v.lp.eq0, v.lp.in0, v.lp.m_eq, r);
            double kz, kx;
            cp_row_sums2(a.ptr[g], a.ptr[g + 1], a.idx, a.val, v.zs, v.xs, ld, &kz, &kx);
            const double bi = a.b[g], yn = cp_dual_point(kz, bi, ld(v.ys + r), a.sigma[g], r >= v.lp.m_eq);
            v.ys[r] = yn;
            rows[0] += cp_gap_row_term(yn, bi);
            rows[1] = cp_gap_violation(rows[1], kx - bi, r < v.lp.m_eq);
        }
        many_post<2, 2>(cpm_red, kCpmWaves, v.tid, rows);
        __syncthreads();  // the barrier that ends the dual half: y is the y of this iteration
        double cols[2] = {0.0, 0.0};  // c x, the bound's column terms
        for (i32 j = v.tid; j < v.n; j += v.W) {
            cols[0] += v.c[j] * ld(v.xs + j);
            cols[1] += cp_gap_col_term(cpm_direction(a, v, ld, j), v.lb[j], v.ub[j]);  // d_j as the next primal half computes it
        }
        many_post<2, 0>(cpm_red + 2 * kCpmWaves, kCpmWaves, v.tid, cols);
        __syncthreads();  // the slots of every wave are written
        ++done;
        until = sp.check_every;
        if (v.tid == 0) {
            double f[4], bound;  // sum y b, violation, c x, column terms: each over the waves in increasing order
            many_fold<4, 2>(cpm_red, kCpmWaves, v.W, f);
            const bool stop = cp_gap_decide(f[2], f[3], f[0], f[1], sp.tol_gap, sp.tol_feas, &bound);
            CpmGap *rec = sp.rec + id;
            rec->primal = f[2];
            rec->bound = bound;
            rec->violation = f[1];
            many_decide(sp.ctl + id, done, stop, cpm_red + 4 * kCpmWaves);
        }
        if (many_decided(cpm_red + 4 * kCpmWaves)) break;
    }
    if ((stages & 2) && v.tid == 0) sp.ctl[id].done = done;
    cpm_close<LDS>(v);
}

// out[5 k + 0..4] as slp_cp_report; one workgroup per LP
__global__ __launch_bounds__(kBlock) void k_cpm_report(CpmArgs a, double *__restrict__ out) {
    __shared__ double lds[kBlock / kWave];
    const CpmLp lp = a.lps[blockIdx.x];
    const i32 m = lp.m_eq + lp.m_in;
    const double *x = a.x + lp.col0, *x4 = a.x4 + lp.col0, *z = a.z + lp.col0, *y = a.y + lp.y0, *c = a.c + lp.col0;
    double s1 = 0.0, s2 = 0.0, veq = -__builtin_inf(), vin = -__builtin_inf(), veqx = -__builtin_inf(), c0 = 0.0, c1 = 0.0;
    for (i32 r = threadIdx.x; r < m; r += kBlock) {
        const i64 g = many_row(lp.eq0, lp.in0, lp.m_eq, r);
        double kx = 0.0, kx4 = 0.0, kz = 0.0;  // three chains in storage order
        for (i64 q = a.ptr[g]; q < a.ptr[g + 1]; ++q) {
            const i32 j = a.idx[q];
            const double v = a.val[q];
            kx += v * x[j];
            kx4 += v * x4[j];
            kz += v * z[j];
        }
        const double bi = a.b[g], yi = y[r];
        s1 += yi * (kx - bi);
        s2 += yi * (kx4 - bi);
        if (r < lp.m_eq) {
            const double e = fabs(kz - bi), ex = fabs(kx - bi);
            veq = e > veq ? e : veq;
            veqx = ex > veqx ? ex : veqx;
        } else {
            const double v = kx - bi;
            vin = v > vin ? v : vin;
        }
    }
    for (i32 j = threadIdx.x; j < lp.n; j += kBlock) {
        const double cj = c[j];
        c0 += cj * x[j];
        c1 += cj * x4[j];
    }
    const double r0 = block_reduce<false>(s1, lds), r1 = block_reduce<false>(s2, lds);
    const double r2 = block_reduce<true>(veq, lds), r3 = block_reduce<true>(vin, lds), r4 = block_reduce<true>(veqx, lds);
    const double r5 = block_reduce<false>(c0, lds), r6 = block_reduce<false>(c1, lds);
    if (threadIdx.x == 0) {
        double *o = out + (i64)blockIdx.x * 5;
        o[0] = r5 + r0;
        o[1] = r6 + r1;
        o[2] = (lp.m_eq > 0) ? (r2 == -__builtin_inf() ? 0.0 : r2) : 0.0;
        o[3] = r3;
        o[4] = (r4 == -__builtin_inf()) ? 0.0 : r4;
    }
}

}  // namespace slp

using namespace slp;

struct slp_cp_many {
    slp_matrix *k = nullptr;  // owned; its index arrays are local to the LPs once the set-up is done
    i64 count = 0, n = 0, m = 0, m_eq = 0;
    double alpha = 1, theta = 1;
    std::vector<CpmLp> lps;
    ManyGroup group[2];  // the LPs of each form
    DevBuf<i32> list[2];
    DevBuf<CpmLp> table;
    DevBuf<double> b, c, lb, ub, t, sigma, x, z, y, x4, out;
    // stopping: off while tol < 0.  The kernel without the test touches no record, so the whole iterations run while it is off
    // are counted here and added to every record when the test is armed (and when the state is read)
    DevBuf<CpmCtl> ctl;
    double tol = -1.0;
    i64 check_every = 1, uncounted = 0;
    // the certificate (slp_many_cpgap_set_stop): off while tol_gap < 0; at most one of the two tests is armed
    DevBuf<CpmGap> gap;
    double tol_gap = -1.0, tol_feas = 0.0;
    // compaction (slp_many_cp_set_compaction): the launches of an armed call run over the live list of each form
    ManyFormLists live;
    i64 cap = kManyMaxItersPerLaunch;  // SLP_CP_MANY_KMAX
    ~slp_cp_many() { delete k; }
};

namespace slp {

static CpmArgs cpm_args(const slp_cp_many *s, int g) {
    const CsrDev &a = s->k->a, &at = s->k->at;
    CpmArgs r;
    r.lps = s->table.p;
    r.list = s->list[g].p;
    r.ptr = a.ptr.p; r.tptr = at.ptr.p;
    r.idx = a.idx.p; r.tidx = at.idx.p;
    r.val = a.val.p; r.tval = at.val.p;
    r.c = s->c.p; r.t = s->t.p; r.lb = s->lb.p; r.ub = s->ub.p; r.b = s->b.p; r.sigma = s->sigma.p;
    r.x = s->x.p; r.z = s->z.p; r.y = s->y.p; r.x4 = s->x4.p;
    r.one_plus_theta = 1.0 + s->theta;
    r.theta = s->theta;
    return r;
}

// one launch of form g over `wgs` workgroups.  LIVE (armed only): over the form's live list, built in front of it
template <bool LDS, bool LIVE>
static void cpm_launch(slp_cp_many *s, int g, CpmArgs a, i64 wgs, int it, int stages, bool store, int stop) {
    const ManyGroup &gr = s->group[g];
    const CpmStop sp = {s->ctl.p, s->tol, s->check_every};
    const dim3 grid((unsigned)wgs), block(gr.block);
    const size_t lds = LDS ? gr.lds_bytes : 0;
    const i32 *live_n = nullptr;
    if (LIVE) {
        many_form_list(s->live, s->group, g, s->table.p, s->ctl.p, s->count);
        a.list = s->live.ids[g].p;
        live_n = s->live.n[g].p;
    }
    if (stop == 2) {
        const CpmGapStop gp = {s->ctl.p, s->gap.p, s->tol_gap, s->tol_feas, s->check_every};
        hipLaunchKernelGGL((k_cpm_iterate_gap<LDS, LIVE>), grid, block, lds, ctx().stream, a, it, stages, (int)store, gp, live_n);
    } else if (stop) hipLaunchKernelGGL((k_cpm_iterate<LDS, true, LIVE>), grid, block, lds, ctx().stream, a, it, stages, (int)store, sp, live_n);
    else hipLaunchKernelGGL((k_cpm_iterate<LDS, false, false>), grid, block, lds, ctx().stream, a, it, stages, (int)store, sp, live_n);
}

// `k` times the stages, in launches of at most kmax iterations per form; with the stopping test that is armed (1 the step, 2 the
// certificate), unless `plain` (the half-iteration timings of slp_cp_many_bench, which are no iterations).  With compaction on an
// armed call reads the records back first (one download; it synchronises): per form its grid is the number of LPs live then, its
// cap that of so many workgroups (many_form_call), and every launch runs over the live list k_many_live builds in front of it -- an
// LP that stops in the call leaves the list at the next launch, the surplus workgroups return at its end.  A form without a live
// LP launches nothing.
static void cpm_run(slp_cp_many *s, i64 k, int stages, bool store, bool plain = false) {
    const int stop = plain ? 0 : (s->tol_gap >= 0.0 ? 2 : (s->tol >= 0.0 ? 1 : 0));
    if (!stop && !plain && (stages & 2)) s->uncounted += k;
    const bool live = stop && s->live.on;
    ManyFormCall call = {};
    if (live && k > 0) call = many_form_call(s->lps, many_read_ctl(s->ctl, s->count, s->uncounted).data(), s->group, ctx().num_cu, s->cap);
    for (int g = 0; g < 2; ++g) {
        const ManyGroup &gr = s->group[g];
        if (gr.ids.empty() || (live && call.live[g] == 0)) continue;
        const CpmArgs a = cpm_args(s, g);
        const i64 wgs = live ? call.live[g] : (i64)gr.ids.size(), cap = live ? call.cap[g] : gr.kmax;
        many_split(k, cap, [&](int it) {
            if (live) {
                if (g == 0) cpm_launch<true, true>(s, g, a, wgs, it, stages, store, stop);
                else cpm_launch<false, true>(s, g, a, wgs, it, stages, store, stop);
            } else {
                if (g == 0) cpm_launch<true, false>(s, g, a, wgs, it, stages, store, stop);
                else cpm_launch<false, false>(s, g, a, wgs, it, stages, store, stop);
            }
            s->live.launched[g] = wgs;
            s->live.cap[g] = cap;
            return it;
        });
    }
}

// what both set_stop calls do behind their argument checks: clear the flags, move the uncounted iterations into the records and
// arm at most one of the two tests (a negative tolerance: off)
static void cpm_arm(slp_cp_many *s, double tol, double tol_gap, double tol_feas, i64 check_every) {
    many_rearm(s->ctl, s->count, &s->uncounted);
    s->tol = tol < 0.0 ? -1.0 : tol;
    s->tol_gap = tol_gap < 0.0 ? -1.0 : tol_gap;
    if (tol >= 0.0 || tol_gap >= 0.0) s->check_every = check_every;
    if (tol_gap >= 0.0) s->tol_feas = tol_feas;
}

// what both *_state calls read out; any pointer may be NULL.  Synchronises.
static void cpm_state(slp_cp_many *s, int64_t *iterations, int32_t *stopped, double *step, double *primal, double *bound, double *violation) {
    const std::vector<CpmCtl> h = many_read_ctl(s->ctl, s->count, s->uncounted);
    std::vector<CpmGap> g(h.size());
    if (primal || bound || violation) s->gap.download(g.data(), g.size());
    for (size_t k = 0; k < h.size(); ++k) {
        many_state_head(h[k], k, iterations, stopped);
        if (step) step[k] = h[k].step;
        if (primal) primal[k] = g[k].primal;
        if (bound) bound[k] = g[k].bound;
        if (violation) violation[k] = g[k].violation;
    }
}

// form per LP, workgroup, LDS and launch cap per form -- from the shapes (and the two environment switches) only
static void cpm_plan(slp_cp_many *s) {
    const int force = many_form_switch("SLP_CP_MANY_FORM");
    const i64 cap = s->cap = many_kmax_switch("SLP_CP_MANY_KMAX", kManyMaxItersPerLaunch);
    std::vector<i64> lds_doubles;
    for (const CpmLp &lp : s->lps) lds_doubles.push_back(2 * (i64)lp.n + lp.m_eq + lp.m_in);
    const std::vector<i32> form =
        many_assign_forms(lds_doubles, kCpmLdsLimit, force, "slp_cp_many_create", "SLP_CP_MANY_FORM", "2 n + m", s->group);
    for (size_t k = 0; k < form.size(); ++k) s->lps[k].form = form[k];
    for (int g = 0; g < 2; ++g) {
        ManyGroup &gr = s->group[g];
        if (gr.ids.empty()) continue;
        i64 widest = 1, doubles = 0;
        for (i32 k : gr.ids) {
            const CpmLp &lp = s->lps[(size_t)k];
            widest = std::max<i64>(widest, std::max<i64>(lp.n, (i64)lp.m_eq + lp.m_in));
            doubles = std::max<i64>(doubles, 2 * (i64)lp.n + lp.m_eq + lp.m_in);
        }
        const int w = many_width(widest, kCpmMaxBlock);
        gr.block = w;
        gr.lds_bytes = g == 0 ? (size_t)doubles * sizeof(double) : 0;
        i64 passes = 1;
        for (i32 k : gr.ids) {
            const CpmLp &lp = s->lps[(size_t)k];
            passes = std::max<i64>(passes, (lp.n + w - 1) / w + ((i64)lp.m_eq + lp.m_in + w - 1) / w);
        }
        gr.passes = passes;
        gr.kmax = many_launch_cap(kManyUnitsPerLaunch, passes, (i64)gr.ids.size(), ctx().num_cu, cap);
    }
}

}  // namespace slp

extern "C" {

int64_t slp_cp_many_lds_limit(void) { return kCpmLdsLimit; }

slp_cp_many *slp_cp_many_create(int64_t count, const int64_t *n, const int64_t *m_eq, const int64_t *m_ineq, const int64_t *indptr,
                                const int32_t *indices, const double *data, const double *b, const double *c, const double *lb,
                                const double *ub, const double *x0, double alpha, double theta) {
    SLP_API_PTR({
        SLP_REQUIRE(count >= 1, "slp_cp_many_create: count must be at least 1");
        SLP_REQUIRE(n && m_eq && m_ineq && indptr && b && c && lb && ub, "slp_cp_many_create: NULL argument");
        // everything below up to the memory check reads the host arrays only: nothing is allocated before the set is known to be
        // well formed and to fit
        auto s = std::unique_ptr<slp_cp_many>(new slp_cp_many());
        s->count = count; s->alpha = alpha; s->theta = theta;
        s->lps.resize((size_t)count);
        i64 N = 0, Me = 0, Mi = 0;
        for (i64 k = 0; k < count; ++k) {
            SLP_REQUIRE(n[k] >= 1 && m_eq[k] >= 0 && m_ineq[k] >= 0 && m_eq[k] + m_ineq[k] >= 1,
                        "slp_cp_many_create: every LP needs at least one variable and one row");
            CpmLp &lp = s->lps[(size_t)k];
            lp.col0 = N; lp.eq0 = Me; lp.in0 = Mi;  // in0: completed below, once the equality rows are counted
            lp.y0 = Me + Mi;
            N += n[k]; Me += m_eq[k]; Mi += m_ineq[k];
            SLP_REQUIRE(N < ((i64)1 << 31) && Me + Mi < ((i64)1 << 31), "slp_cp_many_create: the set has 2^31 or more variables or rows");
            lp.n = (i32)n[k]; lp.m_eq = (i32)m_eq[k]; lp.m_in = (i32)m_ineq[k];
        }
        for (CpmLp &lp : s->lps) lp.in0 += Me;
        const i64 M = Me + Mi;
        s->n = N; s->m = M; s->m_eq = Me;
        std::vector<ManyRows> rows;  // an LP's equality rows, then its inequality rows
        for (i64 k = 0; k < count; ++k) {
            const CpmLp &lp = s->lps[(size_t)k];
            rows.push_back({k, lp.eq0, lp.eq0 + lp.m_eq, lp.col0, lp.col0 + lp.n});
            rows.push_back({k, lp.in0, lp.in0 + lp.m_in, lp.col0, lp.col0 + lp.n});
        }
        many_check_block({"slp_cp_many_create", "indptr", "must be non-decreasing", "", false}, indptr, indices, indices && data, M, rows);
        const i64 nnz = indptr[M];
        cpm_plan(s.get());
        // the CSR pair and the scratch of the device transposition, seven vectors over the columns (x, z, x4, c, lb, ub, T),
        // three over the rows (y, b, Sigma), the table, the lists and the report
        many_require_memory("slp_cp_many_create", count,
                            40.0 * (double)nnz + 16.0 * (double)(N + M + 2) + 8.0 * (7.0 * (double)N + 3.0 * (double)M) +
                                (double)count * (double)(sizeof(CpmLp) + sizeof(CpmCtl) + sizeof(CpmGap) + sizeof(i32) + 5 * sizeof(double)));
        s->k = slp_matrix_create(M, N, indptr, indices, data);
        if (!s->k) throw Error(slp_last_error());
        require_csr(s->k, "slp_cp_many_create");
        build_transpose(s->k);
        s->t.alloc((size_t)N);
        s->sigma.alloc((size_t)M);
        cp_preconditioners_csr(s->k, Me, alpha, s->t.p, s->sigma.p);
        s->table.upload(s->lps.data(), (size_t)count);
        hipLaunchKernelGGL(k_cpm_localise, dim3((unsigned)count), dim3(kBlock), 0, ctx().stream, s->table.p, s->k->a.ptr.p, s->k->a.idx.p,
                           s->k->at.ptr.p, s->k->at.idx.p, Me);
        SLP_HIP(hipGetLastError());
        many_upload_lists(s->group, s->list);
        for (const void *kernel : {reinterpret_cast<const void *>(k_cpm_iterate<true, false, false>),
                                   reinterpret_cast<const void *>(k_cpm_iterate<true, true, false>),
                                   reinterpret_cast<const void *>(k_cpm_iterate<true, true, true>),
                                   reinterpret_cast<const void *>(k_cpm_iterate_gap<true, false>),
                                   reinterpret_cast<const void *>(k_cpm_iterate_gap<true, true>)})
            many_lds_opt_in(kernel, s->group[0].lds_bytes, kCpmLdsLimit * sizeof(double));
        s->c.upload(c, (size_t)N);
        s->lb.upload(lb, (size_t)N);
        s->ub.upload(ub, (size_t)N);
        s->b.upload(b, (size_t)M);
        s->x.alloc((size_t)N);
        if (x0) s->x.upload(x0, (size_t)N);
        else s->x.zero();
        s->z.copy_from(s->x);  // x3 = x (:190)
        s->y.alloc((size_t)M);
        s->y.zero();           // :166,177
        s->x4.alloc((size_t)N);
        s->x4.zero();
        s->out.alloc((size_t)5 * (size_t)count);
        std::vector<CpmCtl> ctl((size_t)count, CpmCtl{{0, 0, 0, 0}, __builtin_inf(), 0.0});
        s->ctl.upload(ctl.data(), ctl.size());
        std::vector<CpmGap> gap((size_t)count, CpmGap{__builtin_inf(), -__builtin_inf(), __builtin_inf()});
        s->gap.upload(gap.data(), gap.size());
        SLP_HIP(hipStreamSynchronize(ctx().stream));
        return s.release();
    })
}

void slp_cp_many_destroy(slp_cp_many *s) { delete s; }

int slp_cp_many_iterate(slp_cp_many *s, int64_t k) {
    SLP_API_INT({
        SLP_REQUIRE(s && k >= 0, "slp_cp_many_iterate: bad arguments");
        cpm_run(s, k, 3, false);
    })
}

int slp_cp_many_primal_step(slp_cp_many *s) { SLP_API_INT({ SLP_REQUIRE(s, "NULL handle"); cpm_run(s, 1, 1, true); }) }

int slp_cp_many_dual_step(slp_cp_many *s) { SLP_API_INT({ SLP_REQUIRE(s, "NULL handle"); cpm_run(s, 1, 2, false); }) }

int slp_cp_many_report(slp_cp_many *s, double *out) {
    SLP_API_INT({
        SLP_REQUIRE(s && out, "slp_cp_many_report: NULL argument");
        hipLaunchKernelGGL(k_cpm_report, dim3((unsigned)s->count), dim3(kBlock), 0, ctx().stream, cpm_args(s, 0), s->out.p);
        SLP_HIP(hipGetLastError());
        s->out.download(out, (size_t)5 * (size_t)s->count);
    })
}

int slp_many_cp_set_stop(slp_cp_many *s, double tol, int64_t check_every) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_cp_set_stop: NULL handle");
        SLP_REQUIRE(tol < 0.0 || (std::isfinite(tol) && check_every >= 1),
                    "slp_many_cp_set_stop: tol must be finite and >= 0 with check_every >= 1 (tol < 0 turns the test off)");
        cpm_arm(s, tol, -1.0, 0.0, check_every);  // arming one test disarms the other
    })
}

int slp_many_cpgap_set_stop(slp_cp_many *s, double tol_gap, double tol_feas, int64_t check_every) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_cpgap_set_stop: NULL handle");
        SLP_REQUIRE(tol_gap < 0.0 || (std::isfinite(tol_gap) && std::isfinite(tol_feas) && tol_feas >= 0.0 && check_every >= 1),
                    "slp_many_cpgap_set_stop: tol_gap and tol_feas must be finite and >= 0 with check_every >= 1 (tol_gap < 0 turns the "
                    "test off)");
        cpm_arm(s, -1.0, tol_gap, tol_feas, check_every);
    })
}

int slp_many_cpgap_state(slp_cp_many *s, int64_t *iterations, int32_t *stopped, double *primal, double *bound, double *violation) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_cpgap_state: NULL handle");
        cpm_state(s, iterations, stopped, nullptr, primal, bound, violation);
    })
}

int slp_many_cp_stop_state(slp_cp_many *s, int64_t *iterations, int32_t *stopped, double *step) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_cp_stop_state: NULL handle");
        cpm_state(s, iterations, stopped, step, nullptr, nullptr, nullptr);
    })
}

int slp_many_cp_set_compaction(slp_cp_many *s, int on) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_cp_set_compaction: NULL handle");
        SLP_REQUIRE(on == 0 || on == 1, "slp_many_cp_set_compaction: on must be 0 or 1");
        if (on) many_form_alloc(s->live, s->group);
        s->live.on = on != 0;
    })
}

int slp_many_cp_live_state(slp_cp_many *s, int64_t live[2], int32_t *order, int64_t launched[2], int64_t cap[2]) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_cp_live_state: NULL handle");
        many_form_state("slp_many_cp_live_state", s->live, s->group, s->table.p, s->ctl.p, s->count, live, order, launched, cap);
    })
}

int slp_cp_many_get_x(slp_cp_many *s, double *x) { SLP_API_INT({ SLP_REQUIRE(s && x, "NULL argument"); s->x.download(x, (size_t)s->n); }) }

int slp_cp_many_get_y(slp_cp_many *s, double *y) { SLP_API_INT({ SLP_REQUIRE(s && y, "NULL argument"); s->y.download(y, (size_t)s->m); }) }

int slp_cp_many_get_preconditioners(slp_cp_many *s, double *t, double *sigma) {
    SLP_API_INT({
        SLP_REQUIRE(s, "NULL handle");
        if (t) s->t.download(t, (size_t)s->n);
        if (sigma) {  // Sigma lies in the row order of K: LP by LP for the caller, as y
            std::vector<double> h((size_t)s->m);
            s->sigma.download(h.data(), (size_t)s->m);
            for (const CpmLp &lp : s->lps) {
                for (i32 r = 0; r < lp.m_eq; ++r) sigma[lp.y0 + r] = h[(size_t)(lp.eq0 + r)];
                for (i32 r = 0; r < lp.m_in; ++r) sigma[lp.y0 + lp.m_eq + r] = h[(size_t)(lp.in0 + r)];
            }
        }
    })
}

int slp_cp_many_form(const slp_cp_many *s, int64_t k) { return (s && k >= 0 && k < s->count) ? s->lps[(size_t)k].form : -1; }

int slp_cp_many_bench(slp_cp_many *s, int64_t k, double ms[3]) {
    SLP_API_INT({
        SLP_REQUIRE(s && k > 0 && ms, "slp_cp_many_bench: bad arguments");
        Context &c = ctx();
        const int stages[3] = {3, 1, 2};
        for (int q = 0; q < 3; ++q) {
            float f = 0.f;
            SLP_HIP(hipEventRecord(c.ev0, c.stream));
            cpm_run(s, k, stages[q], false, q > 0);
            SLP_HIP(hipEventRecord(c.ev1, c.stream));
            SLP_HIP(hipEventSynchronize(c.ev1));
            SLP_HIP(hipEventElapsedTime(&f, c.ev0, c.ev1));
            ms[q] = (double)f / (double)k;
        }
    })
}

}  // extern "C"
