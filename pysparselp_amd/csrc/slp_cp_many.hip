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
// tol_gap * inf holds in IEEE arithmetic; a bound of -inf must not stop).  k_cpm_iterate_gap is the third kind of k_cpm_iterate, a
// template of its own so that the two above stay textually what they were.  An iteration that is no check is the text of STOP =
// false plus two scalar counters.  A check iteration has its own copy of the dual loop -- K x beside K z in one row walk, per lane
// sum y_r b_r over its rows in increasing order and the nan-max of the violation -- then, behind the dual half's barrier, one pass over
// the columns (d_j, its term of the bound, c_j x_j).  A wave reduces its lanes by shuffles in a fixed order (many_wave_sum,
// many_wave_nanmax) into one LDS slot per quantity; behind one more barrier lane 0 folds the waves in increasing order, writes
// the record CpmGap (primal, bound, violation: +inf, -inf, +inf before the first check) and ONE decision slot, and a last barrier
// later every lane reads it.  The two sums are in that fixed order, a function of the shapes only.  done, stopped and stop_iter of
// CpmCtl are shared with the step test; nothing waits in a record between primal_step and dual_step.
#include <algorithm>
#include <cmath>
#include <memory>
#include <type_traits>

#include "slp_cp_shared.h"
#include "slp_kernels.h"
#include "slp_many.h"

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

// per LP, in device memory; written by lane 0 of the LP's workgroup (STOP) and by the host between launches
struct CpmCtl {
    i64 done;       // whole iterations completed
    i64 stop_iter;  // `done` when it stopped
    double step;    // the last evaluated step, +inf before the first test
    double dx;      // the primal half's maximum of a check iteration, carried from primal_step to dual_step
    i32 stopped, pad;
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

// `iters` times the stages of one LP (bit 0 primal half, bit 1 dual half); store: the primal half also writes x4 (:260-261).
// STOP: the stopping test of the header comment; `sp` is not looked at without it.
template <bool LDS, bool STOP>
__global__ __launch_bounds__(kCpmMaxBlock) void k_cpm_iterate(CpmArgs a, int iters, int stages, int store, CpmStop sp) {
    extern __shared__ __attribute__((aligned(16))) double cpm_lds[];
    __shared__ double cpm_red[STOP ? 2 * kCpmWaves + 1 : 1];  // per wave the maxima of the two halves, then the decision
    using LD = typename std::conditional<LDS, CpLoadPlain, CpLoadWorkgroup>::type;
    const LD ld;
    const i32 id = a.list[blockIdx.x];
    const CpmLp lp = a.lps[id];
    const i32 n = lp.n, m = lp.m_eq + lp.m_in, W = (i32)blockDim.x, tid = (i32)threadIdx.x;
    i64 done = 0, until = 0;  // STOP: iterations completed; iterations up to and including the next check
    if (STOP) {
        const CpmCtl *ctl = sp.ctl + id;
        if (ctl->stopped) return;  // set before the launch: the same for every lane
        done = ctl->done;          // lane 0 writes the record only behind a barrier that follows this load
        until = sp.check_every - done % sp.check_every;
    }
    const bool has_eq = lp.m_eq > 0, has_in = lp.m_in > 0;
    double *xg = a.x + lp.col0, *zg = a.z + lp.col0, *yg = a.y + lp.y0;
    double *xs = xg, *zs = zg, *ys = yg;
    if (LDS) {
        xs = cpm_lds;
        zs = xs + n;
        ys = zs + n;
        for (i32 j = tid; j < n; j += W) { xs[j] = xg[j]; zs[j] = zg[j]; }
        for (i32 r = tid; r < m; r += W) ys[r] = yg[r];
        __syncthreads();
    }
    const double *c = a.c + lp.col0, *t = a.t + lp.col0, *lb = a.lb + lp.col0, *ub = a.ub + lp.col0;
    const i64 *tptr = a.tptr + lp.col0;
    for (int it = 0; it < iters; ++it) {
        const bool check = STOP && until == 1;  // uniform: a function of the record and of `it`
        if (stages & 1) {
            double dx = 0.0;
            for (i32 j = tid; j < n; j += W) {
                double se, si;
                cp_column_sums(tptr[j], tptr[j + 1], a.tidx, a.tval, ys, 1, lp.m_eq, ld, &se, &si);
                const double d = cp_direction(c[j], se, si, has_eq, has_in);
                const double xo = ld(xs + j), l = lb[j], u = ub[j];
                double x2, zn;
                cp_primal_point(d, xo, t[j], l, u, a.one_plus_theta, a.theta, &x2, &zn);
                zs[j] = zn;
                xs[j] = x2;
                if (store) a.x4[lp.col0 + j] = (d < 0.0) ? u : l;
                if (STOP) dx = many_nanmax(dx, fabs(x2 - xo));
            }
            if (check) {
                dx = many_wave_nanmax(dx);
                if ((tid & (kWave - 1)) == 0) cpm_red[tid / kWave] = dx;
            }
            __syncthreads();  // same compute unit: the stores of this half are visible to the next one
        }
        if (STOP && !(stages & 2)) {  // primal_step: the reduced dx waits in the record for dual_step
            if (check && tid == 0) {
                double dx = cpm_red[0];
                for (i32 w = 1; w < W / kWave; ++w) dx = many_nanmax(dx, cpm_red[w]);
                sp.ctl[id].dx = dx;
            }
            continue;
        }
        if (stages & 2) {
            double dy = 0.0;
            for (i32 r = tid; r < m; r += W) {
                const i64 g = many_row(lp.eq0, lp.in0, lp.m_eq, r);
                const double kz = cp_row_sum(a.ptr[g], a.ptr[g + 1], a.idx, a.val, zs, 1, ld);
                const double yo = ld(ys + r), yn = cp_dual_point(kz, a.b[g], yo, a.sigma[g], r >= lp.m_eq);
                ys[r] = yn;
                if (STOP) dy = many_nanmax(dy, fabs(yn - yo));
            }
            if (check) {
                dy = many_wave_nanmax(dy);
                if ((tid & (kWave - 1)) == 0) cpm_red[kCpmWaves + tid / kWave] = dy;
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
                CpmCtl *ctl = sp.ctl + id;
                double dx = (stages & 1) ? cpm_red[0] : ctl->dx, dy = cpm_red[kCpmWaves];
                for (i32 w = 1; w < W / kWave; ++w) {
                    if (stages & 1) dx = many_nanmax(dx, cpm_red[w]);
                    dy = many_nanmax(dy, cpm_red[kCpmWaves + w]);
                }
                const double step = many_nanmax(dx, dy);
                const bool stop = step <= sp.tol;  // false for a NaN
                ctl->step = step;
                if (stop) {
                    ctl->stopped = 1;
                    ctl->stop_iter = done;
                }
                cpm_red[2 * kCpmWaves] = stop ? 1.0 : 0.0;
            }
            __syncthreads();  // the one barrier the test adds, in a check iteration only
            if (cpm_red[2 * kCpmWaves] != 0.0) break;  // one slot, read by every lane: uniform
        }
    }
    if (STOP && (stages & 2) && tid == 0) sp.ctl[id].done = done;
    if (LDS) {
        for (i32 j = tid; j < n; j += W) { xg[j] = xs[j]; zg[j] = zs[j]; }
        for (i32 r = tid; r < m; r += W) yg[r] = ys[r];
    }
}

// per LP, beside CpmCtl: the numbers of the last evaluated certificate (+inf, -inf, +inf before the first); written by lane 0 of
// the LP's workgroup in a check iteration of k_cpm_iterate_gap only
struct CpmGap {
    double primal, bound, violation;
};

struct CpmGapStop {
    CpmCtl *ctl;  // done, stopped, stop_iter: shared with the step test; step and dx are not touched
    CpmGap *rec;
    double tol_gap, tol_feas;
    i64 check_every;
};

// min as np.minimum: a NaN on either side stays
__device__ __forceinline__ double cpm_nanmin(double a, double b) { return (b < a || b != b) ? b : a; }

// cp_row_sum with a second chain beside it: K z and K x of one row in one walk, each a single accumulator in storage order
template <class LD>
__device__ __forceinline__ void cpm_row_sums2(i64 s, i64 e, const i32 *__restrict__ idx, const double *__restrict__ val, const double *__restrict__ z,
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

// The third kind of k_cpm_iterate: the iteration of STOP = false with the duality-gap certificate as the per-LP stopping test
// (header comment).  A kernel of its own, so that the two instantiations above stay what they are; the iteration outside a check
// is the text of STOP = false plus two scalar counters, and a check iteration has its own copy of the dual loop.  Every branch
// around a barrier is on `stages`, `check`, the record or the decision slot: uniform.
template <bool LDS>
__global__ __launch_bounds__(kCpmMaxBlock) void k_cpm_iterate_gap(CpmArgs a, int iters, int stages, int store, CpmGapStop sp) {
    extern __shared__ __attribute__((aligned(16))) double cpm_lds[];
    __shared__ double cpm_red[4 * kCpmWaves + 1];  // per wave: sum y b, violation, c x, the bound's column terms; then the decision
    using LD = typename std::conditional<LDS, CpLoadPlain, CpLoadWorkgroup>::type;
    const LD ld;
    const i32 id = a.list[blockIdx.x];
    const CpmLp lp = a.lps[id];
    const i32 n = lp.n, m = lp.m_eq + lp.m_in, W = (i32)blockDim.x, tid = (i32)threadIdx.x;
    const CpmCtl *ctl0 = sp.ctl + id;
    if (ctl0->stopped) return;  // set before the launch: the same for every lane
    i64 done = ctl0->done;      // lane 0 writes the record only behind a barrier that follows this load
    i64 until = sp.check_every - done % sp.check_every;
    const bool has_eq = lp.m_eq > 0, has_in = lp.m_in > 0;
    double *xg = a.x + lp.col0, *zg = a.z + lp.col0, *yg = a.y + lp.y0;
    double *xs = xg, *zs = zg, *ys = yg;
    if (LDS) {
        xs = cpm_lds;
        zs = xs + n;
        ys = zs + n;
        for (i32 j = tid; j < n; j += W) { xs[j] = xg[j]; zs[j] = zg[j]; }
        for (i32 r = tid; r < m; r += W) ys[r] = yg[r];
        __syncthreads();
    }
    const double *c = a.c + lp.col0, *t = a.t + lp.col0, *lb = a.lb + lp.col0, *ub = a.ub + lp.col0;
    const i64 *tptr = a.tptr + lp.col0;
    for (int it = 0; it < iters; ++it) {
        if (stages & 1) {
            for (i32 j = tid; j < n; j += W) {
                double se, si;
                cp_column_sums(tptr[j], tptr[j + 1], a.tidx, a.tval, ys, 1, lp.m_eq, ld, &se, &si);
                const double d = cp_direction(c[j], se, si, has_eq, has_in);
                const double xo = ld(xs + j), l = lb[j], u = ub[j];
                double x2, zn;
                cp_primal_point(d, xo, t[j], l, u, a.one_plus_theta, a.theta, &x2, &zn);
                zs[j] = zn;
                xs[j] = x2;
                if (store) a.x4[lp.col0 + j] = (d < 0.0) ? u : l;
            }
            __syncthreads();  // same compute unit: the stores of this half are visible to the next one
        }
        if (!(stages & 2)) continue;  // primal_step: the certificate needs nothing of this half but x itself
        if (until != 1) {             // no check: the dual half of STOP = false
            for (i32 r = tid; r < m; r += W) {
                const i64 g = many_row(lp.eq0, lp.in0, lp.m_eq, r);
                const double kz = cp_row_sum(a.ptr[g], a.ptr[g + 1], a.idx, a.val, zs, 1, ld);
                ys[r] = cp_dual_point(kz, a.b[g], ld(ys + r), a.sigma[g], r >= lp.m_eq);
            }
            __syncthreads();
            ++done;
            --until;
            continue;
        }
        // a check iteration: the dual half with K x beside K z, then the certificate pass over the columns
        double yb = 0.0, viol = 0.0;
        for (i32 r = tid; r < m; r += W) {
            const i64 g = many_row(lp.eq0, lp.in0, lp.m_eq, r);
            double kz, kx;
            cpm_row_sums2(a.ptr[g], a.ptr[g + 1], a.idx, a.val, zs, xs, ld, &kz, &kx);
            const double bi = a.b[g], yn = cp_dual_point(kz, bi, ld(ys + r), a.sigma[g], r >= lp.m_eq);
            ys[r] = yn;
            if (yn != 0.0) yb += yn * bi;  // the guard keeps 0 * inf out (a row without a finite bound has y = 0)
            const double v = kx - bi;
            viol = many_nanmax(viol, r < lp.m_eq ? fabs(v) : v);
        }
        yb = many_wave_sum(yb);
        viol = many_wave_nanmax(viol);
        if ((tid & (kWave - 1)) == 0) {
            cpm_red[tid / kWave] = yb;
            cpm_red[kCpmWaves + tid / kWave] = viol;
        }
        __syncthreads();  // the barrier that ends the dual half: y is the y of this iteration
        double cx = 0.0, bt = 0.0;
        for (i32 j = tid; j < n; j += W) {
            double se, si;
            cp_column_sums(tptr[j], tptr[j + 1], a.tidx, a.tval, ys, 1, lp.m_eq, ld, &se, &si);
            const double d = cp_direction(c[j], se, si, has_eq, has_in);  // the bits the next primal half computes
            cx += c[j] * ld(xs + j);
            if (d != 0.0) bt += cpm_nanmin(d * lb[j], d * ub[j]);
        }
        cx = many_wave_sum(cx);
        bt = many_wave_sum(bt);
        if ((tid & (kWave - 1)) == 0) {
            cpm_red[2 * kCpmWaves + tid / kWave] = cx;
            cpm_red[3 * kCpmWaves + tid / kWave] = bt;
        }
        __syncthreads();  // the slots of every wave are written
        ++done;
        until = sp.check_every;
        if (tid == 0) {
            double sy = cpm_red[0], vmax = cpm_red[kCpmWaves], primal = cpm_red[2 * kCpmWaves], cols = cpm_red[3 * kCpmWaves];
            for (i32 w = 1; w < W / kWave; ++w) {  // the waves in increasing order
                sy += cpm_red[w];
                vmax = many_nanmax(vmax, cpm_red[kCpmWaves + w]);
                primal += cpm_red[2 * kCpmWaves + w];
                cols += cpm_red[3 * kCpmWaves + w];
            }
            const double bound = cols - sy, gap = fabs(primal - bound);
            // false for a NaN; an infinite gap (bound = -inf) never stops, whatever tol_gap * inf would say
            const bool stop = vmax <= sp.tol_feas && gap < __builtin_inf() && gap <= sp.tol_gap * (1.0 + fabs(primal) + fabs(bound));
            CpmGap *rec = sp.rec + id;
            rec->primal = primal;
            rec->bound = bound;
            rec->violation = vmax;
            if (stop) {
                CpmCtl *ctl = sp.ctl + id;
                ctl->stopped = 1;
                ctl->stop_iter = done;
            }
            cpm_red[4 * kCpmWaves] = stop ? 1.0 : 0.0;
        }
        __syncthreads();
        if (cpm_red[4 * kCpmWaves] != 0.0) break;  // one slot, read by every lane: uniform
    }
    if ((stages & 2) && tid == 0) sp.ctl[id].done = done;
    if (LDS) {
        for (i32 j = tid; j < n; j += W) { xg[j] = xs[j]; zg[j] = zs[j]; }
        for (i32 r = tid; r < m; r += W) yg[r] = ys[r];
    }
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

template <bool LDS>
static void cpm_launch(const slp_cp_many *s, const ManyGroup &gr, const CpmArgs &a, int it, int stages, bool store, int stop) {
    const CpmStop sp = {s->ctl.p, s->tol, s->check_every};
    const dim3 grid((unsigned)gr.ids.size()), block(gr.block);
    const size_t lds = LDS ? gr.lds_bytes : 0;
    if (stop == 2) {
        const CpmGapStop gp = {s->ctl.p, s->gap.p, s->tol_gap, s->tol_feas, s->check_every};
        hipLaunchKernelGGL((k_cpm_iterate_gap<LDS>), grid, block, lds, ctx().stream, a, it, stages, (int)store, gp);
    } else if (stop) hipLaunchKernelGGL((k_cpm_iterate<LDS, true>), grid, block, lds, ctx().stream, a, it, stages, (int)store, sp);
    else hipLaunchKernelGGL((k_cpm_iterate<LDS, false>), grid, block, lds, ctx().stream, a, it, stages, (int)store, sp);
}

// `k` times the stages, in launches of at most kmax iterations per form; with the stopping test that is armed (1 the step, 2 the
// certificate), unless `plain` (the half-iteration timings of slp_cp_many_bench, which are no iterations)
static void cpm_run(slp_cp_many *s, i64 k, int stages, bool store, bool plain = false) {
    const int stop = plain ? 0 : (s->tol_gap >= 0.0 ? 2 : (s->tol >= 0.0 ? 1 : 0));
    if (!stop && !plain && (stages & 2)) s->uncounted += k;
    for (int g = 0; g < 2; ++g) {
        const ManyGroup &gr = s->group[g];
        if (gr.ids.empty()) continue;
        const CpmArgs a = cpm_args(s, g);
        many_split(k, gr.kmax, [&](int it) {
            if (g == 0) cpm_launch<true>(s, gr, a, it, stages, store, stop);
            else cpm_launch<false>(s, gr, a, it, stages, store, stop);
            return it;
        });
    }
}

// the records with the iterations of the unarmed launches added; synchronises
static std::vector<CpmCtl> cpm_read_ctl(slp_cp_many *s) {
    std::vector<CpmCtl> h((size_t)s->count);
    s->ctl.download(h.data(), h.size());
    for (CpmCtl &c : h) c.done += s->uncounted;  // no LP is stopped while the test is off
    return h;
}

// form per LP, workgroup, LDS and launch cap per form -- from the shapes (and the two environment switches) only
static void cpm_plan(slp_cp_many *s) {
    const int force = many_form_switch("SLP_CP_MANY_FORM");
    const i64 cap = many_kmax_switch("SLP_CP_MANY_KMAX", kManyMaxItersPerLaunch);
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
        many_lds_opt_in(reinterpret_cast<const void *>(k_cpm_iterate<true, false>), s->group[0].lds_bytes, kCpmLdsLimit * sizeof(double));
        many_lds_opt_in(reinterpret_cast<const void *>(k_cpm_iterate<true, true>), s->group[0].lds_bytes, kCpmLdsLimit * sizeof(double));
        many_lds_opt_in(reinterpret_cast<const void *>(k_cpm_iterate_gap<true>), s->group[0].lds_bytes, kCpmLdsLimit * sizeof(double));
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
        std::vector<CpmCtl> ctl((size_t)count, CpmCtl{0, 0, __builtin_inf(), 0.0, 0, 0});
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
        std::vector<CpmCtl> h = cpm_read_ctl(s);
        for (CpmCtl &c : h) c.stopped = 0;
        s->ctl.upload(h.data(), h.size());
        s->uncounted = 0;
        s->tol = tol < 0.0 ? -1.0 : tol;
        s->tol_gap = -1.0;  // arming one test disarms the other
        if (tol >= 0.0) s->check_every = check_every;
    })
}

int slp_many_cpgap_set_stop(slp_cp_many *s, double tol_gap, double tol_feas, int64_t check_every) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_cpgap_set_stop: NULL handle");
        SLP_REQUIRE(tol_gap < 0.0 || (std::isfinite(tol_gap) && std::isfinite(tol_feas) && tol_feas >= 0.0 && check_every >= 1),
                    "slp_many_cpgap_set_stop: tol_gap and tol_feas must be finite and >= 0 with check_every >= 1 (tol_gap < 0 turns the "
                    "test off)");
        std::vector<CpmCtl> h = cpm_read_ctl(s);
        for (CpmCtl &c : h) c.stopped = 0;
        s->ctl.upload(h.data(), h.size());
        s->uncounted = 0;
        s->tol = -1.0;  // arming one test disarms the other
        s->tol_gap = tol_gap < 0.0 ? -1.0 : tol_gap;
        if (tol_gap >= 0.0) {
            s->tol_feas = tol_feas;
            s->check_every = check_every;
        }
    })
}

int slp_many_cpgap_state(slp_cp_many *s, int64_t *iterations, int32_t *stopped, double *primal, double *bound, double *violation) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_cpgap_state: NULL handle");
        const std::vector<CpmCtl> h = cpm_read_ctl(s);
        std::vector<CpmGap> g(h.size());
        s->gap.download(g.data(), g.size());
        for (size_t k = 0; k < h.size(); ++k) {
            if (iterations) iterations[k] = h[k].stopped ? h[k].stop_iter : h[k].done;
            if (stopped) stopped[k] = h[k].stopped;
            if (primal) primal[k] = g[k].primal;
            if (bound) bound[k] = g[k].bound;
            if (violation) violation[k] = g[k].violation;
        }
    })
}

int slp_many_cp_stop_state(slp_cp_many *s, int64_t *iterations, int32_t *stopped, double *step) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_cp_stop_state: NULL handle");
        const std::vector<CpmCtl> h = cpm_read_ctl(s);
        for (size_t k = 0; k < h.size(); ++k) {
            if (iterations) iterations[k] = h[k].stopped ? h[k].stop_iter : h[k].done;
            if (stopped) stopped[k] = h[k].stopped;
            if (step) step[k] = h[k].step;
        }
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
