// slp_dga_many.hip -- dual gradient ascent on a LIST of LPs whose constraint matrices differ: one workgroup of 1024 lanes per LP,
// whole iterations inside one launch.  No counterpart in the reference (N solves are N calls of dual_gradient_ascent,
// DualGradientAscent.py:68-245; here each of them is about 30 launches per iteration and bound by launch latency when the LP is
// small).  Every chain of additions is the single solver's (slp_dga_shared.h, included by slp_dga.hip and slp_dga_batch.hip too),
// so LP k is bit for bit what slp_dga computes on LP k alone: x, y, the tie draws taken, the sticky flags and the report.
//
// One iteration of an LP is what dgab_iteration does for one instance, with barriers in place of launch boundaries:
//   column pass : a lane per column: the two masked sums of K^T y in storage order, c_bar, x = the dual argmin      (k_dgab_cols)
//   row pass    : a lane per row: K x, one sequential chain                                                         (row_dot<1>)
//   per kind of rows (inequalities, then equalities; each only if the LP has that kind):
//     gradient pass -- the kDgaParts partial results, computed by the four virtual blocks (4 waves each) of the workgroup, four
//                      parts per round; the parts past the last tile are (0.0, +inf, 0) and are stored as such
//     the block's scalars -- the kDgaParts partial results reduced as one more 256-lane tile
//     d = K^T g, a lane per column; the fused search (dga_fused_body, breakpoints in LDS); the update of y
// Iterates stay in global memory and are re-read across the barriers with workgroup-scope relaxed loads (DgaLoadWorkgroup);
// nothing but the shapes is kept in a register across a barrier.  No atomics between workgroups, no spin waits, no grid barrier:
// a workgroup never waits for another.  Every loop is bounded by the shapes or by `iters`; every barrier is in control flow that
// is uniform over the workgroup (`active` and `frozen` are read by all lanes after a barrier; a frozen LP's workgroup returns
// before its first barrier).
//
// Layout.  All vectors are concatenated LP by LP: c, lb, ub, x, c_bar, d over the columns, b, y, K x, g over the rows with
// [eq; ineq] contiguous per LP.  K_k is CSR over the LP's rows, K_k^T CSR over its columns with rows increasing inside a column
// (the order build_transpose gives the single solver); the index arrays are local to the LP, the pointer arrays hold positions in
// the entry arrays of the whole list.  DgmLp, one per LP, holds its column base, row base, shape, padding and draw offset.
//
// Dynamic LDS: 16 reduction slots, then the search's fused_lds_bytes(npad) for the largest npad of the list.
//
// Launch cap: slp_many_plan.h (switch SLP_DGA_MANY_KMAX).  A pass is the workgroup once over its columns, its rows, a round of the
// gradient pass or a stage of the sort (dgm_passes); a launch also holds no more iterations than the draws on the device allow
// (two per iteration behind the furthest LP).  The cap is a function of the shapes only, whatever test is armed: a check iteration
// with the bound test (below) adds at most one pass over the columns and one over the rows -- ceil((ceil(n / 256) + ceil(m / 256))
// / 4) rounds of 1024 lanes, a lane one column or one row each -- to an iteration that has at least a column and a row pass of its
// own and, per kind of rows, a further column pass, a row pass, the gradient pass, the sort and the scans: less than doubles
// dgm_passes' smallest term, at check iterations only.
//
// Tie draws: all LPs read the one stream of uniform draws, LP k at its own position draw_offset_k + consumed_k (draw_offset_k: the
// draws its default start took).  The device holds a window of the stream from the smallest position on.
// Report, frozen test and start are ordinary launches over (kDgaParts, count) with the shared energy bodies.
//
// Stopping (slp_many_dual_set_stop; off after create).  DgmStop, one per LP in device memory, in an array of its own beside DgaCtl
// (whose layout the single and the batched solver share): iterations completed, the last evaluated step (and bound), the stopped flag (`reason`).
// Iterations of an LP count from 1 over its whole life; y_t = [y_eq; y_ineq] are its multipliers after iteration t, the inequality
// part after its clamp.  step_t = max_r |y_t,r - y_{t-1},r| over all its rows, as np.max (a NaN stays); a kind of rows that does not
// move in iteration t (block predicate false) contributes 0.  At the end of an iteration t with t % check_every == 0 the LP stops
// iff step_t <= tol -- and its sticky NaN bit is down: an LP that has met a NaN breakpoint or step certifies nothing, it runs on.
// The maximum is exact in any order, so the decision is that of a numpy restatement.  The test is the template parameter STOP of
// k_dgm_iterate: STOP = false is the kernel without it, statement by statement, and touches no record (the host counts its
// iterations).  With STOP only a check iteration accumulates anything, in an update loop of its own per kind: a lane the fabs over
// its rows; behind the barrier of the last kind a wave reduces by shuffles into one of the 16 reduction slots, a barrier, lane 0
// folds the slots and writes the step, the count and the flag with ordinary stores, a barrier, and every lane reads the flag with
// a workgroup-scope load: the break is uniform, and so is every barrier.  A stopped LP's workgroup returns before its first
// barrier, as a frozen one (the flag was written by an earlier launch, or behind the barrier before the break: the same for every
// lane); its y, its x (the dual argmin at the top of its last iteration), its tie-draw count and its flags are never written
// again.  The count is read from the record at the start of a launch, so the stopping iteration does not depend on how a run is
// split into calls and launches.
// A stopped LP stands still for ever, so it is no reader of the stream of draws (slp_dga_draws.h): the front of the window moves on
// without it, and the draws behind its position may be gone.  Hence it cannot be resumed: unlike slp_many_cp_set_stop, no call of
// slp_many_dual_set_stop clears a stopped flag.  While an LP is stopped and the test is off, the launch is the kernel with the test
// and a cadence that never comes, so that the LP stays where it is.
//
// A cut-off for the bound (slp_many_dual_set_cutoff, include/slp_hip_ext_dga_many.h): the second template parameter, BOUND.
// <false, false> and <true, false> are the two kernels above.  <true, true>, launched while cut-offs are armed, also evaluates at
// every check of every moving LP bound_t = the dual energy of y_t, bit for bit column 0 of slp_many_dga_report after t iterations,
// and the LP stops iff step_t <= tol (tol >= 0) or bound_t >= targets[k] (targets[k] < +inf) -- the rule of k_dgab_decide; the
// record's `reason` names which (bit 0 step, bit 1 bound), and "stopped" is reason != 0.  The report sums a term per column,
// min(c_bar ub, c_bar lb) where c_bar != 0, and a term per row, y b where y != 0, each alone in lane j % 256 of workgroup j / 256
// of a (kDgaParts, count) x 256 launch (n <= 8192; m <= 65536, which arming with cut-offs checks), block_reduce per workgroup and
// the kDgaParts results added in order on the host.  The kernel forms the same parts with its four virtual blocks, four parts per
// round of dga_block_reduce, and lane 0 adds them in order.  The column terms come from a walk of K^T over the new y that stores
// nothing: x and c_bar stay those of the top of the iteration, which is what a stopped LP keeps.  The parts go through part_min
// (columns) and part_gb (rows), dead behind the last kind's search; no LDS is added, no atomic, no wait.
//
// Compaction (slp_many_dual_set_compaction, include/slp_hip_ext_dga_many_live.h; off after create): the third template parameter,
// LIVE.  Without it a retired LP keeps its workgroup index, and the hardware deals the workgroups of a launch to its eight XCDs in
// turn: with every second LP retired all the live ones sit on four of them.  With compaction on, and an LP that may stand still
// (armed, a stopped LP, or a frozen one), every launch of a call is preceded by k_many_live<DgmIsLive> (slp_many.h: one workgroup
// writes the numbers of the LPs neither frozen nor stopped, in increasing order, and their count) and is <., ., true> over as many
// workgroups as LPs were live when the call began -- the read-back an armed call starts with gives the number; workgroup i takes
// LP ids[i], a workgroup at or past the count returns before its first barrier.  LPs that stop within the call leave the list at
// the next launch, so the survivors stay on consecutive indices.  The cap of the call is that of the live number of workgroups
// (many_live_cap).  An LP's iterations read and write its own data only, so which workgroup runs them changes no bit.
// <., ., false> takes blockIdx.x and never looks at the list: the three kernels above.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "slp_kernels.h"
#include "slp_dga_shared.h"
#include "slp_many.h"
#include "../../include/slp_hip_ext_dga_many.h"
#include "../../include/slp_hip_ext_dga_many_live.h"

using namespace slp;

namespace {

constexpr size_t kDgmSlotBytes = 16 * sizeof(double);   // 4 reduction slots for each of the 4 virtual blocks

struct DgmLp {
    i64 col0, row0;                   // first column (c, lb, ub, x, c_bar, d; rows of K^T), first row (b, y, K x, g; rows of K)
    unsigned long long draw_offset;   // position in the stream of draws of the LP's first tie draw
    i32 n, m_eq, m_in, npad;
};

struct DgmArgs {
    const DgmLp *lps;
    const i64 *ptr, *tptr;    // positions in the entry arrays of the list
    const i32 *idx, *tidx;    // local to the LP
    const double *val, *tval, *b, *c, *lb, *ub;
    double *y, *x, *cbar, *ax, *g, *d, *part_gb, *part_min;
    int *part_any;
    DgaCtl *ctl;
    const double *rnd;
    unsigned long long rnd_base, rnd_count;
};

// per LP, in device memory; written by lane 0 of the LP's workgroup (STOP) and by the host between launches
struct DgmStop {
    i64 done;       // whole iterations completed (the kernel without the test does not count: slp_many_dga::uncounted)
    double step;    // the last evaluated max |y_t - y_{t-1}|, +inf before the first test
    double bound;   // the last evaluated dual energy (BOUND), -inf before the first
    i32 reason, pad;   // bit 0: the step met tol, bit 1: the bound met the cut-off; 0 while the LP is not stopped
};

struct DgmStopArgs {
    DgmStop *rec;
    double tol;               // < 0: the step is evaluated and recorded, not tested (BOUND only)
    const double *targets;    // BOUND: a cut-off per LP, +inf for none
    i64 check_every;
};

// LIVE: the live LPs in increasing order and their number, written by k_many_live<DgmIsLive> in front of the launch
struct DgmLiveArgs {
    const i32 *ids, *n;
};

// an LP is live when it is neither frozen nor stopped: the readers of the stream of draws (dgm_read_ctl, dgm_any_moves)
struct DgmIsLive {
    const DgaCtl *ctl;
    const DgmStop *rec;
    __device__ bool operator()(i32 k) const { return !ctl[k].frozen && !rec[k].reason; }
};

// c_bar of column j of the LP: the two masked sums of K^T y in storage order (k_dgab_cols), then (c + s_eq) + s_ineq
template <class LD>
__device__ __forceinline__ double dgm_cbar(const DgmLp &lp, i32 j, const i64 *tptr, const i32 *tidx, const double *tval, const double *y,
                                           const double *c, LD ld) {
    double se = 0.0, si = 0.0;
    for (i64 q = tptr[j]; q < tptr[j + 1]; ++q) {
        const i32 r = tidx[q];
        const double a = tval[q], yv = ld(y + r);
        se += a * (r < lp.m_eq ? yv : 0.0);
        si += a * (r < lp.m_eq ? 0.0 : yv);
    }
    double cb = c[j];
    if (lp.m_eq > 0) cb = cb + se;
    if (lp.m_in > 0) cb = cb + si;
    return cb;
}

// column j of the LP: c_bar and the dual argmin
template <class LD>
__device__ __forceinline__ void dgm_column(const DgmLp &lp, i32 j, const i64 *tptr, const i32 *tidx, const double *tval, const double *y,
                                           const double *c, const double *lb, const double *ub, double *cbar, double *x, LD ld) {
    const double cb = dgm_cbar(lp, j, tptr, tidx, tval, y, c, ld);
    cbar[j] = cb;
    x[j] = dga_argmin_x(cb, lb[j], ub[j]);
}

// entries s <= q < e of a row times v: storage order, one accumulator (row_dot<1>: loads four entries ahead, adds in order)
template <class LD>
__device__ __forceinline__ double dgm_dot(i64 s, i64 e, const i32 *idx, const double *val, const double *v, LD ld) {
    double acc = 0.0;
    for (i64 k = s; k < e; k += 4) {
        i32 j[4];
        double a[4], xv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const i64 kk = (k + q < e) ? k + q : e - 1;
            j[q] = idx[kk];
            a[q] = val[kk];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) xv[q] = ld(v + j[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (k + q < e) acc += a[q] * xv[q];
    }
    return acc;
}

// `iters` iterations of the LP blockIdx.x.  STOP: the stopping test of the header comment; `sp` is not looked at without it.
// BOUND (with STOP only): a check iteration also evaluates the bound and tests it against the LP's cut-off.
// LIVE: the LP is lv.ids[blockIdx.x], the list k_many_live wrote in front of this launch; a workgroup past its end returns before
// its first barrier (*lv.n is the same for every lane).  `lv` is not looked at without it.
template <bool STOP, bool BOUND, bool LIVE>
__global__ __launch_bounds__(kDgaFusedThreads) void k_dgm_iterate(DgmArgs a, int iters, DgmStopArgs sp, DgmLiveArgs lv) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dgm_lds[];
    const DgaLoadWorkgroup ld;
    if (LIVE && blockIdx.x >= (unsigned)*lv.n) return;
    const unsigned k = LIVE ? (unsigned)lv.ids[blockIdx.x] : blockIdx.x;   // the LP of this workgroup
    const DgmLp lp = a.lps[k];
    DgaCtl *ctl = a.ctl + k;
    if (ctl->frozen) return;   // set before the launch: the same for every lane
    i64 done = 0, until = 0;   // STOP: iterations completed; iterations up to and including the next check
    if (STOP) {
        const DgmStop *rec = sp.rec + k;
        if (rec->reason) return;    // set before the launch: the same for every lane
        done = rec->done;           // lane 0 writes the record only behind a barrier that follows this load
        until = sp.check_every - done % sp.check_every;
    }
    const i32 n = lp.n, m = lp.m_eq + lp.m_in, tid = (i32)threadIdx.x, group = tid >> 8, tl = tid & (kBlock - 1);
    double *slots = reinterpret_cast<double *>(dgm_lds) + 4 * group;
    unsigned char *search_lds = dgm_lds + kDgmSlotBytes;
    const double *c = a.c + lp.col0, *lb = a.lb + lp.col0, *ub = a.ub + lp.col0, *b = a.b + lp.row0;
    double *x = a.x + lp.col0, *cbar = a.cbar + lp.col0, *d = a.d + lp.col0;
    double *y = a.y + lp.row0, *ax = a.ax + lp.row0, *g = a.g + lp.row0;
    const i64 *ptr = a.ptr + lp.row0, *tptr = a.tptr + lp.col0;
    double *part_gb = a.part_gb + (i64)k * kDgaParts, *part_min = a.part_min + (i64)k * kDgaParts;
    int *part_any = a.part_any + (i64)k * kDgaParts;
    // the window of draws as this LP's positions see it: its draw `consumed` is rnd[draw_offset + consumed - rnd_base]
    const double *rnd = a.rnd;
    unsigned long long rnd_base = 0, rnd_count = a.rnd_count;
    if (lp.draw_offset >= a.rnd_base) {
        const unsigned long long skip = lp.draw_offset - a.rnd_base;
        rnd += (skip < rnd_count) ? skip : rnd_count;
        rnd_count = (skip < rnd_count) ? rnd_count - skip : 0;
    } else {
        rnd_base = a.rnd_base - lp.draw_offset;
    }
    // the gradient pass: parts with tiles, four of them per round
    const i32 tiles = (m + kBlock - 1) / kBlock, per = (tiles + kDgaParts - 1) / kDgaParts;
    const i32 rounds = ((tiles + per - 1) / per + 3) / 4;
    for (int it = 0; it < iters; ++it) {
        const bool check = STOP && until == 1;   // uniform: a function of the record and of `it`
        double dy = 0.0;                         // STOP: a lane's max |y_new - y_old| of a check iteration; 0.0 from a kind that stands
        for (i32 j = tid; j < n; j += kDgaFusedThreads) dgm_column(lp, j, tptr, a.tidx, a.tval, y, c, lb, ub, cbar, x, ld);
        __syncthreads();   // same compute unit: the stores of a stage are visible to the next one
        for (i32 i = tid; i < m; i += kDgaFusedThreads) ax[i] = dgm_dot(ptr[i], ptr[i + 1], a.idx, a.val, x, ld);
        __syncthreads();
        for (int kind = 1; kind >= 0; --kind) {   // inequalities first, then equalities
            const int ineq = kind;
            const i32 r0 = ineq ? lp.m_eq : 0, r1 = ineq ? m : lp.m_eq;
            if (r1 == r0) continue;
            for (i32 rd = 0; rd < rounds; ++rd)
                dga_grad_body(m, r0, r1, ineq, ax, b, y, g, part_gb, part_min, part_any, 4 * rd + group, kDgaParts, tl, per, slots, ld);
            for (i32 p = 4 * rounds + tid; p < kDgaParts; p += kDgaFusedThreads) {
                part_gb[p] = 0.0;
                part_min[p] = __builtin_inf();
                part_any[p] = 0;
            }
            __syncthreads();
            dga_begin_body(kDgaParts, part_gb, part_min, part_any, ctl, tl, slots, group == 0, ld);
            __syncthreads();
            if (!ld(&ctl->active)) continue;   // read by all lanes after the barrier
            for (i32 j = tid; j < n; j += kDgaFusedThreads) d[j] = dgm_dot(tptr[j], tptr[j + 1], a.tidx, a.tval, g, ld);
            __syncthreads();
            dga_fused_body(n, lp.npad, d, cbar, lb, ub, ctl, rnd, rnd_base, rnd_count, ineq, search_lds, ld);
            __syncthreads();
            const double t = ld(&ctl->t);
            if (check) {   // a loop of its own: the other one stays the loop of the kernel without the test
                for (i32 i = r0 + tid; i < r1; i += kDgaFusedThreads) {
                    const double yo = ld(y + i), yn = dga_update_y(yo, t, ld(g + i), ineq);
                    y[i] = yn;
                    dy = nan_max(dy, fabs(yn - yo));
                }
            } else {
                for (i32 i = r0 + tid; i < r1; i += kDgaFusedThreads) y[i] = dga_update_y(ld(y + i), t, ld(g + i), ineq);
            }
            __syncthreads();
        }
        if (STOP) {   // here an iteration is complete; the last use of the slots lies behind a barrier
            ++done;
            if (!check) {
                --until;
                continue;
            }
            until = sp.check_every;
            DgmStop *rec = sp.rec + k;
            double *red = reinterpret_cast<double *>(dgm_lds);   // the 16 reduction slots: one per wave
            const i32 cparts = (n + kBlock - 1) / kBlock, parts = cparts + (m + kBlock - 1) / kBlock;
            if (BOUND) {
                // The dual energy of the new y as the report sums it.  There term j of the columns (i of the rows) is alone in lane
                // j % 256 of workgroup j / 256 (n <= 8192 and m <= 65536 = kDgaParts * kBlock, which arming has checked): the
                // lane's 0.0 + term, a block_reduce per workgroup, the workgroups' results added in order from 0.0.  Here a part
                // is one virtual block's dga_block_reduce, four parts per round: first the column parts (the walk of dgm_column on
                // the new y; nothing is stored to x or c_bar, which stay those of the top of this iteration), then the row parts.
                // part_min and part_gb of the gradient pass are dead here -- every iteration writes all of them before it reads
                // one -- and take the column and the row parts.  The loop is bounded by the shape: uniform, and so are its barriers.
                for (i32 p0 = 0; p0 < parts; p0 += 4) {
                    const i32 p = p0 + group;
                    double term = 0.0;
                    if (p < cparts) {
                        const i32 j = p * kBlock + tl;
                        if (j < n) {
                            const double cb = dgm_cbar(lp, j, tptr, a.tidx, a.tval, y, c, ld);
                            if (cb != 0.0) {
                                const double u = cb * ub[j], l = cb * lb[j];
                                term = 0.0 + ((u < l) ? u : l);   // the report's lane starts from acc = 0.0: a term of -0.0 becomes +0.0
                            }
                        }
                    } else if (p < parts) {
                        const i32 i = (p - cparts) * kBlock + tl;
                        if (i < m) {
                            const double yi = ld(y + i);
                            if (yi != 0.0) term = 0.0 + yi * b[i];
                        }
                    }
                    const double s = dga_block_reduce<false>(term, tl, slots);
                    if (tl == 0 && p < cparts) part_min[p] = s;
                    else if (tl == 0 && p < parts) part_gb[p - cparts] = s;
                }
            }
            dy = many_wave_nanmax(dy);
            if ((tid & (kWave - 1)) == 0) red[tid / kWave] = dy;
            __syncthreads();
            if (tid == 0) {
                double step = red[0];
                for (int w = 1; w < kDgaFusedThreads / kWave; ++w) step = nan_max(step, red[w]);
                if (BOUND) {
                    // the report's sequential sums of its kDgaParts partial results (dga_bound_finish).  Its parts past the last
                    // term are +0.0, and a sum that starts at +0.0 is never -0.0 (no term is), so adding them changes no bit: the
                    // fold ends at the last used part.
                    double e = 0.0, yb = 0.0;
                    for (i32 p = 0; p < cparts; ++p) e += ld(part_min + p);
                    for (i32 p = 0; p < parts - cparts; ++p) yb += ld(part_gb + p);
                    const double bound = e - yb, target = sp.targets[k];
                    const bool sound = !(ctl->flags & DGA_NAN);   // an LP that has met a NaN breakpoint or step certifies nothing
                    int reason = (sound && sp.tol >= 0.0 && step <= sp.tol) ? 1 : 0;            // false for a NaN
                    if (sound && target < __builtin_inf() && bound >= target) reason |= 2;      // false for a NaN
                    rec->step = step;
                    rec->bound = bound;
                    rec->done = done;
                    rec->reason = reason;
                } else {
                    const int stop = (step <= sp.tol && !(ctl->flags & DGA_NAN)) ? 1 : 0;   // false for a NaN
                    rec->step = step;
                    rec->done = done;
                    rec->reason = stop;
                }
            }
            __syncthreads();   // the two barriers the test adds, in a check iteration only
            if (ld(&rec->reason)) break;   // read by all lanes after the barrier: uniform
        }
    }
    if (STOP && tid == 0) sp.rec[k].done = done;
}

// ---- start, frozen test and report: ordinary launches over (.., count) --------------------------------------------------------

__global__ __launch_bounds__(kBlock) void k_dgm_cols(DgmArgs a, double *__restrict__ cbar, double *__restrict__ x) {
    const DgmLp lp = a.lps[blockIdx.y];
    for (i32 j = blockIdx.x * blockDim.x + threadIdx.x; j < lp.n; j += gridDim.x * blockDim.x)
        dgm_column(lp, j, a.tptr + lp.col0, a.tidx, a.tval, a.y + lp.row0, a.c + lp.col0, a.lb + lp.col0, a.ub + lp.col0, cbar + lp.col0,
                   x + lp.col0, DgaLoadPlain());
}

__global__ __launch_bounds__(kBlock) void k_dgm_rows(DgmArgs a, const double *__restrict__ x, double *__restrict__ out) {
    const DgmLp lp = a.lps[blockIdx.y];
    const i64 *ptr = a.ptr + lp.row0;
    for (i32 i = blockIdx.x * blockDim.x + threadIdx.x; i < lp.m_eq + lp.m_in; i += gridDim.x * blockDim.x)
        out[lp.row0 + i] = dgm_dot(ptr[i], ptr[i + 1], a.idx, a.val, x + lp.col0, DgaLoadPlain());
}

__global__ void k_dgm_energy_x(DgmArgs a, const double *__restrict__ cbar, double *__restrict__ part) {
    __shared__ double red[kBlock / kWave];
    const DgmLp lp = a.lps[blockIdx.y];
    dga_energy_x_body(lp.n, cbar + lp.col0, a.lb + lp.col0, a.ub + lp.col0, part + (i64)blockIdx.y * 4 * kDgaParts, red);
}

__global__ void k_dgm_energy_y(DgmArgs a, const double *__restrict__ ax, double *__restrict__ part) {
    __shared__ double red[kBlock / kWave];
    const DgmLp lp = a.lps[blockIdx.y];
    dga_energy_y_body(lp.m_eq + lp.m_in, lp.m_eq, a.y + lp.row0, a.b + lp.row0, ax + lp.row0, part + (i64)blockIdx.y * 4 * kDgaParts + kDgaParts,
                      red);
}

}  // namespace

struct slp_many_dga {
    i64 count = 0, n = 0, m = 0;   // LPs, all columns, all rows
    i32 max_n = 1, max_m = 1, max_npad = 64;
    i64 kmax = 1;                  // iterations one launch may hold
    i64 passes = 1, kmax_switch = 1;   // what kmax was made of: the passes of the largest LP, the SLP_DGA_MANY_KMAX switch
    std::vector<DgmLp> lps;
    DevBuf<DgmLp> table;
    DevBuf<i64> ptr, tptr;
    DevBuf<i32> idx, tidx;
    DevBuf<double> val, tval, b, c, lb, ub, y, x, cbar, ax, g, d, rcbar, rx, rax, rpart, part_gb, part_min;
    DevBuf<int> part_any;
    DevBuf<DgaCtl> ctl;
    // the shared stream of tie draws
    DevBuf<double> rnd;
    DgaDrawWindow draws;   // the host's view of rnd (slp_dga_draws.h)
    i64 iters = 0;
    StageTimer timer;
    // stopping: the step test is off while tol < 0, the bound test while has_targets is false; off when both are.  The kernel
    // without the test touches no record, so the iterations it runs are counted here and added to the record of every moving LP
    // when the test is armed (and when the state is read)
    DevBuf<DgmStop> stop;
    DevBuf<double> targets;   // a cut-off per LP, allocated at the first arming with cut-offs
    double tol = -1.0;
    bool has_targets = false;
    i64 check_every = 1, uncounted = 0;
    bool any_stopped = false;   // from now on every launch is the kernel with the test: a stopped LP stays where it is
    // compaction (slp_many_dual_set_compaction; off after create): the launches of a call run over the list of the live LPs
    DevBuf<i32> live, live_n;   // allocated at the first use: `count` entries and one
    bool compact = false, any_frozen = false;
    i64 launched = 0, call_cap = 0;   // the grid of the last iteration launch, the cap of the last iterate call that launched
};

namespace {

DgmArgs dgm_args(const slp_many_dga *s) {
    DgmArgs r;
    r.lps = s->table.p;
    r.ptr = s->ptr.p; r.tptr = s->tptr.p;
    r.idx = s->idx.p; r.tidx = s->tidx.p;
    r.val = s->val.p; r.tval = s->tval.p;
    r.b = s->b.p; r.c = s->c.p; r.lb = s->lb.p; r.ub = s->ub.p;
    r.y = s->y.p; r.x = s->x.p; r.cbar = s->cbar.p; r.ax = s->ax.p; r.g = s->g.p; r.d = s->d.p;
    r.part_gb = s->part_gb.p; r.part_min = s->part_min.p; r.part_any = s->part_any.p;
    r.ctl = s->ctl.p;
    r.rnd = s->rnd.p;
    r.rnd_base = s->draws.base;
    r.rnd_count = s->draws.size();
    return r;
}

// workgroup passes of one iteration of an LP: from its shape only
i64 dgm_passes(const DgmLp &lp) {
    const i64 w = kDgaFusedThreads, n = lp.n, m = (i64)lp.m_eq + lp.m_in;
    const i64 cols = (n + w - 1) / w, rows = (m + w - 1) / w;
    const i64 tiles = (m + kBlock - 1) / kBlock, per = (tiles + kDgaParts - 1) / kDgaParts;
    const i64 grad = (((tiles + per - 1) / per + 3) / 4) * per;
    i64 stages = 0;
    for (i64 size = 2; size <= lp.npad; size <<= 1)
        for (i64 stride = size >> 1; stride > 0; stride >>= 1) ++stages;
    const i64 sort = stages * std::max<i64>(1, lp.npad / (2 * w));
    const i64 scans = 8 * ((n + 4 * kDgaTile - 1) / (4 * kDgaTile));
    const i64 kinds = (lp.m_eq > 0) + (lp.m_in > 0);
    return cols + rows + kinds * (grad + 1 + cols + sort + scans + rows);
}

void dgm_plan(slp_many_dga *s) {
    const i64 cap = many_kmax_switch("SLP_DGA_MANY_KMAX", kManyMaxItersPerLaunch);
    i64 passes = 1;
    for (const DgmLp &lp : s->lps) passes = std::max(passes, dgm_passes(lp));
    s->kmax = many_launch_cap(kManyUnitsPerLaunch, passes, s->count, ctx().num_cu, cap);
    s->passes = passes;
    s->kmax_switch = cap;
}

size_t dgm_lds_bytes(const slp_many_dga *s) { return kDgmSlotBytes + fused_lds_bytes(s->max_npad); }

dim3 dgm_grid(i64 work, i64 count) { return dim3((unsigned)std::max<i64>(1, (work + kBlock - 1) / kBlock), (unsigned)count); }

// c_bar and x of the multipliers into (cbar, x), for every LP
void dgm_argmin(slp_many_dga *s, double *cbar, double *x) {
    hipLaunchKernelGGL(k_dgm_cols, dgm_grid(s->max_n, s->count), dim3(kBlock), 0, ctx().stream, dgm_args(s), cbar, x);
    SLP_HIP(hipGetLastError());
}

void dgm_report(slp_many_dga *s, double *out) {
    hipStream_t st = ctx().stream;
    const size_t sc = (size_t)s->count;
    if (!s->rcbar.p) { s->rcbar.alloc((size_t)s->n); s->rx.alloc((size_t)s->n); s->rax.alloc((size_t)s->m); s->rpart.alloc((size_t)4 * kDgaParts * sc); }
    const DgmArgs a = dgm_args(s);
    dgm_argmin(s, s->rcbar.p, s->rx.p);
    hipLaunchKernelGGL(k_dgm_rows, dgm_grid(s->max_m, s->count), dim3(kBlock), 0, st, a, s->rx.p, s->rax.p);
    hipLaunchKernelGGL(k_dgm_energy_x, dim3(kDgaParts, (unsigned)sc), dim3(kBlock), 0, st, a, s->rcbar.p, s->rpart.p);
    hipLaunchKernelGGL(k_dgm_energy_y, dim3(kDgaParts, (unsigned)sc), dim3(kBlock), 0, st, a, s->rax.p, s->rpart.p);
    SLP_HIP(hipGetLastError());
    std::vector<double> h((size_t)4 * kDgaParts * sc);
    s->rpart.download(h.data(), h.size());
    for (size_t k = 0; k < sc; ++k) dga_report_finish(h.data() + k * 4 * kDgaParts, true, out + 3 * k);
}

// the controls of all LPs and, in `r` if given, their stop records with the iterations of the launches without the test added;
// refreshes the bound on the positions in the stream of draws.  A frozen LP and a stopped one stand still: no readers of the stream.
void dgm_read_ctl(slp_many_dga *s, std::vector<DgaCtl> &h, std::vector<DgmStop> *r = nullptr) {
    h.resize((size_t)s->count);
    s->ctl.download(h.data(), (size_t)s->count);
    std::vector<DgmStop> own;
    std::vector<DgmStop> &rec = r ? *r : own;
    rec.resize((size_t)s->count);
    s->stop.download(rec.data(), (size_t)s->count);
    for (size_t k = 0; k < rec.size(); ++k)
        if (!h[k].frozen && !rec[k].reason) rec[k].done += s->uncounted;
    s->draws.observe(dga_furthest_reader(
        h.size(), [&](size_t k) { return !h[k].frozen && !rec[k].reason; },
        [&](size_t k) { return (uint64_t)(s->lps[k].draw_offset + h[k].consumed); }));
}

bool dgm_any_moves(const std::vector<DgaCtl> &h, const std::vector<DgmStop> &rec) {
    for (size_t k = 0; k < h.size(); ++k)
        if (!h[k].frozen && !rec[k].reason) return true;
    return false;
}

// the rule of the stopping test from now on: tol < 0 = no step test, targets == NULL = no bound test; both checked by the caller
void dgm_set_rule(slp_many_dga *s, double tol, const double *targets, i64 check_every) {
    std::vector<DgaCtl> h;
    std::vector<DgmStop> rec;
    dgm_read_ctl(s, h, &rec);   // synchronises; the iterations of the launches without the test are in the records now
    s->stop.upload(rec.data(), rec.size());
    s->uncounted = 0;
    s->any_stopped = false;
    for (const DgmStop &r : rec) s->any_stopped = s->any_stopped || r.reason;   // the marks stay: a stopped LP cannot be resumed
    if (targets) s->targets.upload(targets, (size_t)s->count);
    s->has_targets = targets != nullptr;
    s->tol = tol < 0.0 ? -1.0 : tol;
    if (tol >= 0.0 || targets) s->check_every = check_every;
}

void dgm_live_alloc(slp_many_dga *s) {
    if (s->live.p) return;
    s->live.alloc((size_t)s->count);
    s->live_n.alloc(1);
}

// the list of the live LPs from the flags as they are on the device, behind everything enqueued so far
void dgm_live_list(slp_many_dga *s) {
    dgm_live_alloc(s);
    hipLaunchKernelGGL(k_many_live<DgmIsLive>, dim3(1), dim3(kManyLiveLanes), 0, ctx().stream, DgmIsLive{s->ctl.p, s->stop.p}, (i32)s->count,
                       s->live.p, s->live_n.p);
}

template <bool LIVE>
void dgm_launch(slp_many_dga *s, bool stop, i64 grid, int it, const DgmStopArgs &sp) {
    const dim3 g((unsigned)grid), block(kDgaFusedThreads);
    const DgmLiveArgs lv = {s->live.p, s->live_n.p};
    hipStream_t st = ctx().stream;
    if (s->has_targets) hipLaunchKernelGGL((k_dgm_iterate<true, true, LIVE>), g, block, dgm_lds_bytes(s), st, dgm_args(s), it, sp, lv);
    else if (stop) hipLaunchKernelGGL((k_dgm_iterate<true, false, LIVE>), g, block, dgm_lds_bytes(s), st, dgm_args(s), it, sp, lv);
    else hipLaunchKernelGGL((k_dgm_iterate<false, false, LIVE>), g, block, dgm_lds_bytes(s), st, dgm_args(s), it, sp, lv);
}

}  // namespace

extern "C" {

slp_many_dga *slp_many_dga_create(int64_t count, const int64_t *n, const int64_t *m_eq, const int64_t *m_ineq, const int64_t *indptr,
                                  const int32_t *indices, const double *data, const double *b, const double *c, const double *lb,
                                  const double *ub, const double *y0, const int64_t *draw_offset) {
    SLP_API_PTR({
        SLP_REQUIRE(count >= 1, "slp_many_dga_create: count must be at least 1");
        SLP_REQUIRE(count <= 65535, "slp_many_dga_create: at most 65535 LPs");
        SLP_REQUIRE(n && m_eq && m_ineq && indptr && b && c && lb && ub && y0 && draw_offset, "slp_many_dga_create: NULL argument");
        // everything below up to the memory check reads the host arrays only: nothing is allocated or launched before the list is
        // known to be well formed and to fit
        auto s = std::unique_ptr<slp_many_dga>(new slp_many_dga());
        s->count = count;
        s->lps.resize((size_t)count);
        i64 N = 0, M = 0;
        for (i64 k = 0; k < count; ++k) {
            if (n[k] > kDgaFusedMax)
                throw Error("slp_many_dga_create: LP " + std::to_string(k) + " has " + std::to_string(n[k]) + " variables; the list form holds at most " +
                            std::to_string(kDgaFusedMax) + " per LP (an LP with more belongs to the single solver, slp_dga_create_on)");
            if (n[k] < 1 || m_eq[k] < 0 || m_ineq[k] < 0 || m_eq[k] + m_ineq[k] < 1)
                throw Error("slp_many_dga_create: LP " + std::to_string(k) + " needs at least one variable and one constraint row");
            SLP_REQUIRE(draw_offset[k] >= 0, "slp_many_dga_create: a negative draw offset");
            DgmLp &lp = s->lps[(size_t)k];
            lp.col0 = N; lp.row0 = M;
            N += n[k]; M += m_eq[k] + m_ineq[k];
            SLP_REQUIRE(N < ((i64)1 << 31) && M < ((i64)1 << 31), "slp_many_dga_create: the list has 2^31 or more variables or rows");
            SLP_REQUIRE(m_eq[k] + m_ineq[k] < ((i64)1 << 31) - kBlock, "slp_many_dga_create: an LP has too many rows");
            lp.n = (i32)n[k]; lp.m_eq = (i32)m_eq[k]; lp.m_in = (i32)m_ineq[k];
            lp.draw_offset = (unsigned long long)draw_offset[k];
            int npad = 64;
            while (npad < lp.n) npad <<= 1;
            lp.npad = npad;
            s->max_n = std::max(s->max_n, lp.n);
            s->max_m = std::max(s->max_m, lp.m_eq + lp.m_in);
            s->max_npad = std::max(s->max_npad, npad);
        }
        s->n = N; s->m = M;
        std::vector<ManyRows> rows;
        for (i64 k = 0; k < count; ++k) {
            const DgmLp &lp = s->lps[(size_t)k];
            rows.push_back({k, lp.row0, lp.row0 + lp.m_eq + lp.m_in, 0, lp.n});
        }
        many_check_block({"slp_many_dga_create", "indptr", "must be non-decreasing", "", true}, indptr, indices, indices && data, M, rows);
        const i64 nnz = indptr[M];
        SLP_REQUIRE(nnz < ((i64)1 << 31), "slp_many_dga_create: the list has 2^31 or more entries");
        dgm_plan(s.get());
        // both orientations (20 B an entry), the pointers, ten vectors over the columns (c, lb, ub, x, c_bar, d and the report's
        // two), seven over the rows, per LP the table, the controls and the partial results of the pass and of the report
        many_require_memory("slp_many_dga_create", count,
                            24.0 * (double)nnz + 8.0 * (double)(N + M + 2) + 8.0 * (8.0 * (double)N + 7.0 * (double)M) +
                                (double)count * (double)(sizeof(DgmLp) + sizeof(DgaCtl) + sizeof(DgmStop) + 8.0 * 7.0 * kDgaParts));
        // K_k^T on the host: a counting transposition per LP walks its rows in order, so rows increase inside a column
        std::vector<i64> tptr((size_t)N + 1, 0);
        std::vector<i32> tidx((size_t)nnz);
        std::vector<double> tval((size_t)nnz);
        {
            std::vector<i64> fill;
            for (const DgmLp &lp : s->lps) {
                const i64 m = (i64)lp.m_eq + lp.m_in, q0 = indptr[lp.row0], q1 = indptr[lp.row0 + m];
                fill.assign((size_t)lp.n + 1, 0);
                for (i64 q = q0; q < q1; ++q) ++fill[(size_t)indices[q] + 1];
                fill[0] = q0;
                for (i32 j = 0; j < lp.n; ++j) fill[(size_t)j + 1] += fill[(size_t)j];
                for (i32 j = 0; j <= lp.n; ++j) tptr[(size_t)(lp.col0 + j)] = fill[(size_t)j];
                for (i64 r = 0; r < m; ++r)
                    for (i64 q = indptr[lp.row0 + r]; q < indptr[lp.row0 + r + 1]; ++q) {
                        const i64 at = fill[(size_t)indices[q]]++;
                        tidx[(size_t)at] = (i32)r;
                        tval[(size_t)at] = data[q];
                    }
            }
        }
        const size_t sn = (size_t)N, sm = (size_t)M, sc = (size_t)count, sz = (size_t)nnz;
        s->table.upload(s->lps.data(), sc);
        s->ptr.upload(indptr, sm + 1);
        s->tptr.upload(tptr.data(), sn + 1);
        s->idx.alloc(sz); s->val.alloc(sz); s->tidx.alloc(sz); s->tval.alloc(sz);
        if (sz) { s->idx.upload(indices, sz); s->val.upload(data, sz); s->tidx.upload(tidx.data(), sz); s->tval.upload(tval.data(), sz); }
        s->b.upload(b, sm); s->c.upload(c, sn); s->lb.upload(lb, sn); s->ub.upload(ub, sn); s->y.upload(y0, sm);
        s->x.alloc(sn); s->cbar.alloc(sn); s->d.alloc(sn); s->ax.alloc(sm); s->g.alloc(sm);
        s->part_gb.alloc((size_t)kDgaParts * sc); s->part_min.alloc((size_t)kDgaParts * sc); s->part_any.alloc((size_t)kDgaParts * sc);
        s->rnd.alloc(1);
        s->ctl.alloc(sc);
        s->ctl.zero();
        for (const void *kernel :
             {reinterpret_cast<const void *>(k_dgm_iterate<false, false, false>), reinterpret_cast<const void *>(k_dgm_iterate<true, false, false>),
              reinterpret_cast<const void *>(k_dgm_iterate<true, true, false>), reinterpret_cast<const void *>(k_dgm_iterate<false, false, true>),
              reinterpret_cast<const void *>(k_dgm_iterate<true, false, true>), reinterpret_cast<const void *>(k_dgm_iterate<true, true, true>)})
            SLP_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kDgmSlotBytes + fused_lds_bytes(kDgaFusedMax))));
        {
            const std::vector<DgmStop> rec(sc, DgmStop{0, __builtin_inf(), -__builtin_inf(), 0, 0});
            s->stop.upload(rec.data(), sc);
        }
        dgm_argmin(s.get(), s->cbar.p, s->x.p);   // the x of y0: what a frozen LP keeps
        // a start whose dual energy is -inf freezes its LP (the single solve returns at once, :133-139)
        std::vector<double> rep(3 * sc);
        dgm_report(s.get(), rep.data());
        std::vector<DgaCtl> h(sc);
        memset(h.data(), 0, sc * sizeof(DgaCtl));
        for (size_t k = 0; k < sc; ++k) h[k].frozen = rep[3 * k] == -INFINITY;
        for (size_t k = 0; k < sc; ++k) s->any_frozen = s->any_frozen || h[k].frozen;
        s->ctl.upload(h.data(), sc);
        dgm_read_ctl(s.get(), h);
        return s.release();
    })
}

void slp_many_dga_destroy(slp_many_dga *s) { delete s; }

int64_t slp_many_dga_kmax(const slp_many_dga *s) { return s ? s->kmax : -1; }

int slp_many_dga_iterate(slp_many_dga *s, int64_t k) {
    SLP_API_INT({
        SLP_REQUIRE(s && k >= 0, "slp_many_dga_iterate: bad arguments");
        // with the test: armed, or off with an LP that has to stay stopped (a cadence that never comes)
        const bool armed = s->tol >= 0.0 || s->has_targets, stop = armed || s->any_stopped;
        // over the list of the live LPs: compaction is on and an LP may stand still
        bool live = s->compact && (stop || s->any_frozen);
        const DgmStopArgs sp = {s->stop.p, s->tol, s->targets.p, armed ? s->check_every : INT64_MAX};
        i64 grid = s->count, cap = s->kmax;
        if (stop || live) {   // when every LP is stopped or frozen nothing is launched and the count of iterations stays
            std::vector<DgaCtl> h;
            std::vector<DgmStop> rec;
            dgm_read_ctl(s, h, &rec);
            if (!dgm_any_moves(h, rec)) {
                if (stop) return 0;
                live = false;   // never armed and every LP frozen: the launches of a state without compaction, which count
            }
            if (live) {
                // the LPs live now: the grid of every launch of this call (an LP that stops in it is known here at the next call;
                // its workgroup index goes to the survivors, the surplus workgroups return at the list's end) and its cap
                grid = 0;
                for (size_t j = 0; j < h.size(); ++j) grid += !h[j].frozen && !rec[j].reason;
                cap = many_live_cap(s->passes, grid, ctx().num_cu, s->kmax_switch);
            }
        }
        s->call_cap = cap;
        many_split(k, cap, [&](int want) {
            // at most two tie draws per LP and iteration: iterations the buffer cannot run dry in
            const int it = (int)s->draws.reserve(want);
            if (it < 1) return it;
            s->timer.mark(-1);
            if (live) {
                dgm_live_list(s);
                dgm_launch<true>(s, stop, grid, it, sp);
            } else {
                dgm_launch<false>(s, stop, grid, it, sp);
            }
            s->timer.mark(ST_FUSED);
            s->launched = grid;
            s->iters += it;
            if (!stop) s->uncounted += it;
            return it;
        });
    })
}

int slp_many_dga_push_random(slp_many_dga *s, const double *draws, int64_t count) {
    SLP_API_INT({
        SLP_REQUIRE(s && count >= 0 && (draws || count == 0), "slp_many_dga_push_random: bad arguments");
        std::vector<DgaCtl> h;
        std::vector<DgmStop> rec;
        dgm_read_ctl(s, h, &rec);
        // (an LP never reaches what lies before its offset: the start of the stream went into the default starts)
        dga_push_draws(h, [s](size_t k) { return s->lps[k].draw_offset; }, [&](size_t k) { return !h[k].frozen && !rec[k].reason; }, s->draws,
                       s->rnd, draws, count, kAppendFirst);
    })
}

int slp_many_dga_status(slp_many_dga *s, int64_t *out) {
    SLP_API_INT({
        SLP_REQUIRE(s && out, "slp_many_dga_status: NULL argument");
        std::vector<DgaCtl> h;
        dgm_read_ctl(s, h);
        dga_status_out(h, s->draws, s->iters, out);
    })
}

int slp_many_dga_frozen(slp_many_dga *s, int32_t *out) {
    SLP_API_INT({
        SLP_REQUIRE(s && out, "slp_many_dga_frozen: NULL argument");
        std::vector<DgaCtl> h;
        dgm_read_ctl(s, h);
        dga_frozen_out(h, out);
    })
}

int slp_many_dga_get_x(slp_many_dga *s, double *x) { SLP_API_INT({ SLP_REQUIRE(s && x, "NULL argument"); s->x.download(x, (size_t)s->n); }) }

int slp_many_dga_get_y(slp_many_dga *s, double *y) { SLP_API_INT({ SLP_REQUIRE(s && y, "NULL argument"); s->y.download(y, (size_t)s->m); }) }

int slp_many_dga_report(slp_many_dga *s, double *out) {
    SLP_API_INT({
        SLP_REQUIRE(s && out, "slp_many_dga_report: NULL argument");
        dgm_report(s, out);
    })
}

int slp_many_dual_set_stop(slp_many_dga *s, double tol, int64_t check_every) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_dual_set_stop: NULL handle");
        SLP_REQUIRE(tol < 0.0 || (std::isfinite(tol) && check_every >= 1),
                    "slp_many_dual_set_stop: tol must be finite and >= 0 with check_every >= 1 (tol < 0 turns the test off)");
        dgm_set_rule(s, tol, nullptr, check_every);
    })
}

int slp_many_dual_set_cutoff(slp_many_dga *s, double tol, const double *targets, int64_t check_every) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_dual_set_cutoff: NULL handle");
        SLP_REQUIRE(tol < 0.0 || std::isfinite(tol), "slp_many_dual_set_cutoff: tol must be finite (tol < 0: no step test)");
        SLP_REQUIRE((tol < 0.0 && !targets) || check_every >= 1, "slp_many_dual_set_cutoff: check_every must be at least 1");
        if (targets) {   // nothing is launched or changed before the cut-offs and the shapes are known to be in range
            for (i64 k = 0; k < s->count; ++k) {
                SLP_REQUIRE(targets[k] == targets[k] && targets[k] != -INFINITY,
                            "slp_many_dual_set_cutoff: a cut-off is a number or +inf (none for that LP), not NaN or -inf");
                const i64 m = (i64)s->lps[(size_t)k].m_eq + s->lps[(size_t)k].m_in;
                if (m > (i64)kDgaParts * kBlock)
                    throw Error("slp_many_dual_set_cutoff: LP " + std::to_string(k) + " has " + std::to_string(m) + " rows; the bound test holds at most " +
                                std::to_string(kDgaParts * kBlock) + " per LP (the step test alone has no such limit)");
            }
        }
        dgm_set_rule(s, tol, targets, check_every);
    })
}

int slp_many_dual_stop_state(slp_many_dga *s, int64_t *iterations, int32_t *stopped, double *step) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_dual_stop_state: NULL handle");
        std::vector<DgaCtl> h;
        std::vector<DgmStop> rec;
        dgm_read_ctl(s, h, &rec);
        for (size_t k = 0; k < rec.size(); ++k) {
            if (iterations) iterations[k] = rec[k].done;   // 0 for a frozen LP: its workgroup returns before it counts
            if (stopped) stopped[k] = rec[k].reason != 0;
            if (step) step[k] = rec[k].step;
        }
    })
}

int slp_many_dual_cutoff_state(slp_many_dga *s, int64_t *iterations, int32_t *reason, double *step, double *bound) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_dual_cutoff_state: NULL handle");
        std::vector<DgaCtl> h;
        std::vector<DgmStop> rec;
        dgm_read_ctl(s, h, &rec);
        for (size_t k = 0; k < rec.size(); ++k) {
            if (iterations) iterations[k] = rec[k].done;   // 0 for a frozen LP: its workgroup returns before it counts
            if (reason) reason[k] = rec[k].reason;
            if (step) step[k] = rec[k].step;
            if (bound) bound[k] = rec[k].bound;
        }
    })
}

int slp_many_dual_set_compaction(slp_many_dga *s, int on) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_dual_set_compaction: NULL handle");
        SLP_REQUIRE(on == 0 || on == 1, "slp_many_dual_set_compaction: on must be 0 or 1");
        if (on) dgm_live_alloc(s);
        s->compact = on != 0;
    })
}

int slp_many_dual_live_state(slp_many_dga *s, int64_t *live, int32_t *order, int64_t *launched, int64_t *cap) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_dual_live_state: NULL handle");
        dgm_live_list(s);
        SLP_HIP(hipGetLastError());
        i32 n = 0;
        s->live_n.download(&n, 1);   // synchronises
        SLP_REQUIRE(n >= 0 && n <= s->count, "slp_many_dual_live_state: the device's count of live LPs is out of range");
        if (live) *live = n;
        if (order) {
            s->live.download(order, (size_t)n);
            std::fill(order + n, order + s->count, -1);
        }
        if (launched) *launched = s->launched;
        if (cap) *cap = s->call_cap;
    })
}

int slp_many_dga_timing(slp_many_dga *s, int on) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_many_dga_timing: NULL handle");
        s->timer.set(on);
    })
}

int slp_many_dga_timing_read(slp_many_dga *s, double out[5]) {
    SLP_API_INT({
        SLP_REQUIRE(s && out, "slp_many_dga_timing_read: NULL argument");
        s->timer.read(out);
    })
}

}  // extern "C"
