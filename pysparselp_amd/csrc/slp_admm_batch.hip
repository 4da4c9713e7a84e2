// slp_admm_batch.hip -- batched ADMM with the projected Gauss-Seidel x-step: B instances of ONE constraint structure.
// No counterpart in the reference (single-threaded numpy: B solves are B calls of lp_admm, ADMM.py:47-269).  The instances share
// the standard-form A, M = gamma_eq A^T A + gamma_ineq I, A^T b, the Gauss-Seidel plan (level order, 1 / diag) and the slack
// bounds: all of it depends on the constraints only and is built once by the set-up chain of slp_admm_create_lp
// (slp_admm_shared.h).  Per instance there is c, hence q = -c + gamma_eq A^T b, and optionally lb, ub, x0 of the original
// variables.  One iteration of an instance, with the expressions and the summation order of slp_admm in SLP_ORDER_SEQUENTIAL
// (every dot product by one lane, in storage order, one accumulator):
//   y_j = ((q_j + gamma_ineq xp_j) - (A^T lambda)_j) - 0                         k_admm_rhs<1>          [ADMM.py:148]
//   level by level: v = w (y_i - sum_k x[idx_k] val_k) invd + x_i, clamped       k_gs_level<true>       [gaussSiedel.pyx:131-152]
//   lambda_i += gamma_eq ((A x)_i - b_i)                                         k_admm_multiplier<1>   [ADMM.py:261-263]
// xp is max(x0, 0) before the first multiplier step and x afterwards (:98, :259).  w = 1 (:162): the factor is left out, 1.0 * t
// is t bit for bit; so is the subtraction of lambda_ineq = +0.
//
// Layout (as slp_cp_batch.hip).  Bt is the instance-tile width, the batch is padded to Bp = Bt * ntiles instances.  A batched
// vector over len elements lies tile by tile, the instance fastest inside a tile:  v(j, k) at ((k / Bt) * len + j) * Bt + k % Bt
// (x, y, q, xp0 over N = n + m_ineq; lambda over m; c over n; lb, ub over N when they differ per instance, one shared vector
// otherwise).  Lanes of padding instances are idle in every kernel: their state stays as allocated (zero).
//
// Two forms of the iteration, the same arithmetic (admm_rhs_one / admm_sweep_one / admm_mult_one of slp_admm_iter.h):
//   tile    k_admmb_tile: ONE workgroup of 1024 lanes owns a tile and runs k whole iterations of its instances in one launch;
//           stages and levels are separated by __syncthreads(), x / y / lambda stay in global memory and are re-read across the
//           barriers with workgroup-scope relaxed loads (as k_gs_sweep_one_block).  No atomics between workgroups, no spin
//           waits, no grid barrier: a workgroup never waits for another.  A lane is one (row of the level, instance of the tile).
//   levels  k_admmb_rhs, one k_admmb_level per dependency level, k_admmb_mult: plain launches over (row, instance) lanes of all
//           tiles -- for few wide levels, where one compute unit per tile would leave the chip idle.
// admmb_choose() picks form and tile width from the shapes and B; SLP_ADMM_BATCH_FORM=tile|levels forces the form
// (SLP_ADMM_BATCH_TILE=1|2|..|64 the width: timing runs).
//
// Report (:213-248), per instance: row pass r = A x - b -> sum r^2, sum lambda r, max |r|; column pass -> c.x, sum (x - xp)^2,
// max -x.  Row i (column j) belongs to slice i mod S; a slice adds its terms in increasing i, one lane per instance adds the S
// slice sums in increasing slice order (k_cpb_report_*); maxima are exact in any order.
//
// Stopping per instance (slp_admm_batch_set_stop, slp_hip_ext_admm_batch.h): the rule of slp_many_admm_set_stop with the batch
// semantics of slp_cp_batch_set_stop_gap.  The state counts its whole iterations t on the host (bumped where a multiplier half
// is enqueued) and hands the count to every launch, so whether an iteration is a check iteration is uniform over a launch's
// lanes and the stopping iteration does not depend on how a run is split into launches or calls.  AdmmbCtl, one per padded
// instance in device memory: the stopped flag (set for padding instances at the first arming), the stopping iteration, the last
// evaluated residual and step, and the reduced step of a sweep whose multiplier half has not run yet.  The test is the template
// parameter STOP of the iteration kernels: STOP = false is the kernel without the test, the only one a never-armed state
// launches.  With STOP a lane reads its instance's flag first and does no other load for a stopped instance, and only a check
// iteration accumulates anything, in loops of its own: fabs(new - old) over the lane's rows of all levels, fabs((A x)_i - b_i)
// -- the value the multiplier update forms -- over its rows of the multiplier pass, both by nan_max (slp_cp_gap.h), exact in
// any order.
//   tile    the lanes of an instance lie BT apart in a wave: shuffles down to BT, one LDS slot per (wave, instance), and behind
//           the multiplier pass's barrier lane k of wave 0 folds the 16 slots of instance k, writes the record and decides.
//           Wave 0 then posts who goes on (one flag per instance, one for the tile) and every lane reads both behind the ONE
//           barrier the test adds to a check iteration; a tile without a running instance returns (uniform: no barrier is
//           left behind), as it does at the start of a launch.
//   levels  in a check iteration every workgroup of a level (of the multiplier pass) reduces its lanes the same way and lane k
//           folds the result into (writes) slot part[(q S + blockIdx.x) Bp + instance], q = 0 step, 1 residual -- a slot belongs
//           to one workgroup index, the launches of a stream follow each other, so no atomic is needed; the step slots are
//           zeroed on the stream before the sweep.  k_admmb_decide, one workgroup per instance behind the multiplier kernel,
//           folds the slots, writes the record and decides.
// Right-hand sides per instance (slp_admm_batch_set_rhs, slp_hip_ext_batch_rhs.h; before the first iteration).  The row scalings
// of the set-up chain depend on the matrices only, so the instances keep sharing the chain, M and its plan; the call scales the
// caller's rows with the kept scalings (k_admmb_scale_rhs) and rebuilds per instance b (tiled like lambda: AdmmbArgs::b_b, the
// template parameter BB of the kernels that read b in every iteration), A^T b_k with the set-up's product, q_k (k_admmb_q) and
// the slack part of lb / ub (k_admmb_scatter_tail; the bound becomes tiled over N if it was shared).
// `running` counts the real instances that go on (an integer atomic decrement where one stops): an armed state reads it once
// at the start of iterate / multiplier_step and enqueues nothing when it is 0.  Nothing else is read back.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "slp_common.h"
#include "slp_cp_gap.h"
#include "slp_kernels.h"
#include "slp_admm_iter.h"
#include "slp_admm_shared.h"
#include "../../include/slp_hip_ext_admm_batch.h"
#include "../../include/slp_hip_ext_batch_rhs.h"

namespace slp {

constexpr int kAdmmbBlock = 1024;     // lanes of the tile form's workgroup
constexpr int kAdmmbMaxSlices = 1024;
constexpr i64 kAdmmbUnitsPerLaunch = 8192;  // workgroup passes (a few microseconds each) one launch of the tile form may hold

struct AdmmbArgs {
    i64 N, m, n, B, nlevels;
    const i64 *tptr; const i32 *tidx; const double *tval;   // rows of A^T
    const i64 *aptr; const i32 *aidx; const double *aval;   // rows of A
    const i64 *gptr; const i32 *gidx; const double *gval; const double *ginvd; const i32 *grows; const i64 *lptr;  // M, level order
    const double *b;                                        // [m], or tiled like lambda (b_b)
    const double *q, *c, *lb, *ub, *xp0;
    double *x, *y, *lam;
    int lb_b, ub_b, xp0_b, b_b;                             // 1: tiled per instance, 0: one shared vector
    double gamma_eq, gamma_ineq;
};

// the record of one (padded) instance and what a launch of a STOP kernel is told about the test (header comment)
struct AdmmbCtl {
    i64 stop_iter;               // t when it stopped
    i32 stopped, pad;            // padding instances: stopped from the first arming on
    double residual, step, dx;   // the last evaluated ones; the reduced step of a sweep that waits for its multiplier half
};
struct AdmmbStop {
    AdmmbCtl *ctl;
    i32 *running;                // real instances that still run
    i64 t0, check_every;         // whole iterations completed when the launch starts; 0: no iteration is a check iteration
    double tol_residual, tol_step;
};

// the workgroup-scope relaxed load of slp_admm_iter.h: a value another lane of the workgroup may have stored before the last barrier
__device__ __forceinline__ double admmb_ld(const double *p) { return AdmmLoadWorkgroup()(p); }

// the three steps for (row, instance k of the tile): the addresses of the tiled layout around the arithmetic of slp_admm_iter.h
template <int BT>
__device__ __forceinline__ void admmb_rhs_one(const AdmmbArgs &a, i64 tile, int k, i64 j, bool first) {
    const i64 o = (tile * a.N + j) * BT + k;
    const double *xp = first ? a.xp0 + (a.xp0_b ? o : j) : a.x + o;
    a.y[o] = admm_rhs_one<BT>(a.tptr[j], a.tptr[j + 1], a.tidx, a.tval, a.lam + tile * a.m * BT + k, a.q + o, xp, !first, a.gamma_ineq,
                              AdmmLoadWorkgroup());  // :148
}

// returns |new - old| of the row, for a check iteration of the stopping test
template <int BT>
__device__ __forceinline__ double admmb_sweep_one(const AdmmbArgs &a, i64 tile, int k, i64 t) {
    const i64 i = a.grows[t];
    const i64 o = (tile * a.N + i) * BT + k;
    const double bi = admmb_ld(a.y + o), xi = admmb_ld(a.x + o), inv = a.ginvd[t];
    const double l = a.lb[a.lb_b ? o : i], u = a.ub[a.ub_b ? o : i];
    const double v = admm_sweep_one<BT>(a.gptr[t], a.gptr[t + 1], a.gidx, a.gval, a.x + tile * a.N * BT + k, bi, xi, inv, l, u, AdmmLoadWorkgroup());
    a.x[o] = v;
    return fabs(v - xi);
}

// BB: b is tiled like lambda (after slp_admm_batch_set_rhs with a batched b_eq); a template parameter, so that a state with a
// shared b launches the code it launched before the switch existed
template <int BT, bool BB>
__device__ __forceinline__ void admmb_mult_one(const AdmmbArgs &a, i64 tile, int k, i64 i) {
    const i64 o = (tile * a.m + i) * BT + k;
    a.lam[o] = admm_mult_one<BT>(a.aptr[i], a.aptr[i + 1], a.aidx, a.aval, a.x + tile * a.N * BT + k, a.lam + o, a.b + (BB ? o : i), a.gamma_eq,
                                 AdmmLoadWorkgroup());  // :261-263
}

// admmb_mult_one of a check iteration: the same lambda_i; returns |(A x)_i - b_i| as the update forms it
template <int BT, bool BB>
__device__ __forceinline__ double admmb_mult_res_one(const AdmmbArgs &a, i64 tile, int k, i64 i) {
    const i64 o = (tile * a.m + i) * BT + k;
    double res;
    a.lam[o] = admm_mult_res_one<BT>(a.aptr[i], a.aptr[i + 1], a.aidx, a.aval, a.x + tile * a.N * BT + k, a.lam + o, a.b + (BB ? o : i), a.gamma_eq,
                                     AdmmLoadWorkgroup(), &res);
    return fabs(res);
}

// ---- the reductions of the stopping test.  The lanes of instance k of a tile are those with threadIdx.x % BT == k: in a wave
// they lie BT apart, so shuffles down to BT leave lane k < BT with the wave's nan_max for instance k; slots[wave * BT + k].
// Every lane of the workgroup calls it (a lane without a row, or of a stopped instance, with 0.0); read behind a later barrier.
template <int BT>
__device__ __forceinline__ void admmb_post(double *slots, double v) {
#pragma unroll
    for (int off = kWave / 2; off >= BT; off >>= 1) v = nan_max(v, __shfl_down(v, off, kWave));
    const int lane = threadIdx.x & (kWave - 1);
    if (lane < BT) slots[(threadIdx.x / kWave) * BT + lane] = v;
}

// the slots of instance k folded over the NW waves of the workgroup
template <int BT, int NW>
__device__ __forceinline__ double admmb_fold(const double *slots, int k) {
    double v = slots[k];
#pragma unroll
    for (int w = 1; w < NW; ++w) v = nan_max(v, slots[w * BT + k]);
    return v;
}

// lane 0 of a workgroup's deciding lanes for one instance, at the end of check iteration t: the record, and one instance fewer
// runs when it stops.  False for a NaN on either side.
__device__ __forceinline__ bool admmb_decide(const AdmmbStop &sp, AdmmbCtl *ctl, i64 t, double residual, double step) {
    ctl->residual = residual;
    ctl->step = step;
    const bool stop = residual <= sp.tol_residual && step <= sp.tol_step;
    if (stop) {
        ctl->stopped = 1;
        ctl->stop_iter = t;
        atomicSub(sp.running, 1);
    }
    return stop;
}

// wave 0 of the tile form (lane k < BT speaks for instance k) posts go[k] = `goes` and go[BT] = any of them; every lane reads
// them behind the barrier: false when no instance of the tile runs, the same for every lane
template <int BT>
__device__ __forceinline__ bool admmb_post_go(int *go, bool goes) {
    if (threadIdx.x < kWave) {
        const bool mine = threadIdx.x < BT && goes;
        if (threadIdx.x < BT) go[threadIdx.x] = mine;
        const bool any = __any(mine);
        if (threadIdx.x == 0) go[BT] = any;
    }
    __syncthreads();
    return go[BT] != 0;
}

// ---- tile form: `iters` iterations of one tile in one workgroup.  stages: bit 0 right-hand side + sweep, bit 1 multiplier.
// STOP: the stopping test of the header comment; `sp` is not looked at without it.  BB: admmb_mult_one's.
template <int BT, bool STOP, bool BB>
__global__ __launch_bounds__(kAdmmbBlock) void k_admmb_tile(AdmmbArgs a, int iters, int first, int stages, AdmmbStop sp) {
    constexpr int kWaves = kAdmmbBlock / kWave;
    __shared__ double red[STOP ? 2 * kWaves * BT : 1];  // step, residual: a slot per (wave, instance).  Unused without STOP: dropped
    __shared__ int go[STOP ? BT + 1 : 1];
    const int k = threadIdx.x & (BT - 1);
    const i64 tile = blockIdx.x;
    const i64 g = threadIdx.x / BT;
    constexpr i64 ng = kAdmmbBlock / BT;
    bool active = STOP ? !sp.ctl[tile * BT + k].stopped : tile * BT + k < a.B;
    if (STOP && !admmb_post_go<BT>(go, active)) return;
    for (int it = 0; it < iters; ++it) {
        const bool check = STOP && sp.check_every > 0 && (sp.t0 + it + 1) % sp.check_every == 0;  // uniform over the launch
        if (stages & 1) {
            if (active)
                for (i64 j = g; j < a.N; j += ng) admmb_rhs_one<BT>(a, tile, k, j, first && it == 0);
            __syncthreads();
            double dx = 0.0;  // a lane without a row in any level contributes 0.0
            for (i64 l = 0; l < a.nlevels; ++l) {
                const i64 beg = a.lptr[l], end = a.lptr[l + 1];
                if (check) {  // a loop of its own: the other one stays the loop of the kernel without the test
                    if (active)
                        for (i64 t = beg + g; t < end; t += ng) dx = nan_max(dx, admmb_sweep_one<BT>(a, tile, k, t));
                } else {
                    if (active)
                        for (i64 t = beg + g; t < end; t += ng) admmb_sweep_one<BT>(a, tile, k, t);
                }
                __syncthreads();  // same compute unit: the stores of this level are visible to the next one
            }
            if (check) admmb_post<BT>(red, dx);  // read behind the multiplier pass's barrier, or behind the one below
        }
        if (STOP && !(stages & 2)) {  // sweep_step: the reduced step waits in the record for multiplier_step
            if (check) {
                __syncthreads();
                if (threadIdx.x < BT && active) sp.ctl[tile * BT + k].dx = admmb_fold<BT, kWaves>(red, k);
            }
            continue;
        }
        if (stages & 2) {
            if (check) {
                double dr = 0.0;  // 0.0 without rows
                if (active)
                    for (i64 i = g; i < a.m; i += ng) dr = nan_max(dr, admmb_mult_res_one<BT, BB>(a, tile, k, i));
                admmb_post<BT>(red + kWaves * BT, dr);
            } else {
                if (active)
                    for (i64 i = g; i < a.m; i += ng) admmb_mult_one<BT, BB>(a, tile, k, i);
            }
            __syncthreads();
        }
        if (STOP && check) {  // here iteration t0 + it + 1 is complete
            bool goes = false;
            if (threadIdx.x < BT && active) {  // lane k of wave 0 decides for instance k
                AdmmbCtl *ctl = sp.ctl + tile * BT + k;
                const double step = (stages & 1) ? admmb_fold<BT, kWaves>(red, k) : ctl->dx;
                goes = !admmb_decide(sp, ctl, sp.t0 + it + 1, admmb_fold<BT, kWaves>(red + kWaves * BT, k), step);
            }
            if (!admmb_post_go<BT>(go, goes)) return;  // the one barrier the test adds to a whole iteration
            active = go[k] != 0;
        }
    }
}

// ---- levels form: lanes over (row, instance) of all tiles; blockIdx.y is the tile.  STOP: a lane of a stopped instance returns
// before its first load; `ctl` is not looked at without it.
template <int BT, bool STOP>
__global__ __launch_bounds__(kBlock) void k_admmb_rhs(AdmmbArgs a, int first, const AdmmbCtl *__restrict__ ctl) {
    const int k = threadIdx.x & (BT - 1);
    const i64 tile = blockIdx.y;
    if (STOP ? ctl[tile * BT + k].stopped != 0 : tile * BT + k >= a.B) return;
    const i64 ng = (i64)gridDim.x * kBlock / BT;
    for (i64 j = ((i64)blockIdx.x * kBlock + threadIdx.x) / BT; j < a.N; j += ng) admmb_rhs_one<BT>(a, tile, k, j, first != 0);
}

// a check iteration's workgroup: the lanes' `v` reduced per instance of the tile; lane k < BT returns true with the result in *out.
// Every lane of the workgroup calls it
template <int BT>
__device__ __forceinline__ bool admmb_block_nanmax(double v, double *out) {
    constexpr int kWaves = kBlock / kWave;
    __shared__ double slots[kWaves * BT];
    admmb_post<BT>(slots, v);
    __syncthreads();
    if (threadIdx.x >= BT) return false;
    *out = admmb_fold<BT, kWaves>(slots, (int)threadIdx.x);
    return true;
}

// part: NULL outside a check iteration; else the step slots [gridDim.x of the widest level x Bp], zeroed before the sweep
template <int BT, bool STOP>
__global__ __launch_bounds__(kBlock) void k_admmb_level(AdmmbArgs a, i64 beg, i64 end, const AdmmbCtl *__restrict__ ctl, i64 Bp,
                                                        double *part) {
    const int k = threadIdx.x & (BT - 1);
    const i64 tile = blockIdx.y;
    const i64 ng = (i64)gridDim.x * kBlock / BT;
    if (!STOP || !part) {
        if (STOP ? ctl[tile * BT + k].stopped != 0 : tile * BT + k >= a.B) return;
        for (i64 t = beg + ((i64)blockIdx.x * kBlock + threadIdx.x) / BT; t < end; t += ng) admmb_sweep_one<BT>(a, tile, k, t);
        return;
    }
    const bool live = !ctl[tile * BT + k].stopped;  // every lane stays for the barrier
    double dx = 0.0;
    if (live)
        for (i64 t = beg + ((i64)blockIdx.x * kBlock + threadIdx.x) / BT; t < end; t += ng) dx = nan_max(dx, admmb_sweep_one<BT>(a, tile, k, t));
    double v;
    if (admmb_block_nanmax<BT>(dx, &v) && live) {
        double *slot = part + (i64)blockIdx.x * Bp + tile * BT + k;  // this workgroup index's own, level after level
        *slot = nan_max(*slot, v);
    }
}

// part: NULL outside a check iteration; else the residual slots [gridDim.x x Bp].  BB: admmb_mult_one's
template <int BT, bool STOP, bool BB>
__global__ __launch_bounds__(kBlock) void k_admmb_mult(AdmmbArgs a, const AdmmbCtl *__restrict__ ctl, i64 Bp, double *__restrict__ part) {
    const int k = threadIdx.x & (BT - 1);
    const i64 tile = blockIdx.y;
    const i64 ng = (i64)gridDim.x * kBlock / BT;
    if (!STOP || !part) {
        if (STOP ? ctl[tile * BT + k].stopped != 0 : tile * BT + k >= a.B) return;
        for (i64 i = ((i64)blockIdx.x * kBlock + threadIdx.x) / BT; i < a.m; i += ng) admmb_mult_one<BT, BB>(a, tile, k, i);
        return;
    }
    const bool live = !ctl[tile * BT + k].stopped;
    double dr = 0.0;
    if (live)
        for (i64 i = ((i64)blockIdx.x * kBlock + threadIdx.x) / BT; i < a.m; i += ng) dr = nan_max(dr, admmb_mult_res_one<BT, BB>(a, tile, k, i));
    double v;
    if (admmb_block_nanmax<BT>(dr, &v) && live) part[(i64)blockIdx.x * Bp + tile * BT + k] = v;
}

// one workgroup per real instance, behind the multiplier kernel of a check iteration t (sp.t0) -- or behind the sweep of a
// sweep_step, where the folded step goes into the record and waits: the nstep step slots and the nres residual slots (at `res`)
// folded by nan_max, the record, the decision.  stages as in admmb_run.
__global__ __launch_bounds__(kBlock) void k_admmb_decide(i64 Bp, i64 nstep, const double *__restrict__ step, i64 nres,
                                                         const double *__restrict__ res, int stages, AdmmbStop sp) {
    constexpr int kWaves = kBlock / kWave;
    __shared__ double slots[2 * kWaves];
    const i64 inst = blockIdx.x;
    AdmmbCtl *ctl = sp.ctl + inst;
    if (ctl->stopped) return;  // the same for every lane
    double dx = 0.0, dr = 0.0;
    if (stages & 1)
        for (i64 g = threadIdx.x; g < nstep; g += kBlock) dx = nan_max(dx, step[g * Bp + inst]);
    if (stages & 2)
        for (i64 g = threadIdx.x; g < nres; g += kBlock) dr = nan_max(dr, res[g * Bp + inst]);
    admmb_post<1>(slots, dx);
    admmb_post<1>(slots + kWaves, dr);
    __syncthreads();
    if (threadIdx.x != 0) return;
    dx = admmb_fold<1, kWaves>(slots, 0);
    if (!(stages & 2)) {
        ctl->dx = dx;
        return;
    }
    admmb_decide(sp, ctl, sp.t0, admmb_fold<1, kWaves>(slots + kWaves, 0), (stages & 1) ? dx : ctl->dx);
}

// ---- report.  part[(q * S + slice) * Bp + instance], S = gridDim.x * 256 / BT slices
//   rows: q = 0 sum r^2, 1 sum lambda r, 2 max |r|       columns: q = 0 sum c x, 1 sum (x - xp)^2, 2 max -x
template <int BT>
__global__ __launch_bounds__(kBlock) void k_admmb_report_rows(AdmmbArgs a, i64 Bp, double *__restrict__ part) {
    const int k = threadIdx.x & (BT - 1);
    const i64 tile = blockIdx.y;
    const i64 group = ((i64)blockIdx.x * kBlock + threadIdx.x) / BT, ng = (i64)gridDim.x * kBlock / BT;
    const i64 inst = tile * BT + k;
    double s0 = 0.0, s1 = 0.0, mx = -__builtin_inf();
    if (inst < a.B)
        for (i64 i = group; i < a.m; i += ng) {
            const double ax = admm_dot<BT>(a.aptr[i], a.aptr[i + 1], a.aidx, a.aval, a.x + tile * a.N * BT + k, AdmmLoadWorkgroup());
            const double r = ax - a.b[a.b_b ? (tile * a.m + i) * BT + k : i];
            s0 += r * r;
            s1 += a.lam[(tile * a.m + i) * BT + k] * r;
            const double ar = fabs(r);
            mx = ar > mx ? ar : mx;
        }
    part[(0 * ng + group) * Bp + inst] = s0;
    part[(1 * ng + group) * Bp + inst] = s1;
    part[(2 * ng + group) * Bp + inst] = mx;
}

template <int BT>
__global__ __launch_bounds__(kBlock) void k_admmb_report_cols(AdmmbArgs a, int first, i64 Bp, double *__restrict__ part) {
    const int k = threadIdx.x & (BT - 1);
    const i64 tile = blockIdx.y;
    const i64 group = ((i64)blockIdx.x * kBlock + threadIdx.x) / BT, ng = (i64)gridDim.x * kBlock / BT;
    const i64 inst = tile * BT + k;
    double s0 = 0.0, s1 = 0.0, mx = -__builtin_inf();
    if (inst < a.B)
        for (i64 j = group; j < a.N; j += ng) {
            const i64 o = (tile * a.N + j) * BT + k;
            const double xj = a.x[o];
            const double dx = first ? xj - a.xp0[a.xp0_b ? o : j] : 0.0;  // xp is x itself after the first multiplier step
            if (j < a.n) s0 += a.c[(tile * a.n + j) * BT + k] * xj;      // the slack columns cost nothing
            s1 += dx * dx;
            mx = (-xj) > mx ? (-xj) : mx;
        }
    part[(0 * ng + group) * Bp + inst] = s0;
    part[(1 * ng + group) * Bp + inst] = s1;
    part[(2 * ng + group) * Bp + inst] = mx;
}

// one lane per instance: the slice sums in increasing slice order; out[3 inst + 0..2] as slp_admm_report
__global__ void k_admmb_report_final(i64 B, i64 Bp, i64 srows, const double *__restrict__ rp, i64 scols, const double *__restrict__ cp,
                                     double gamma_eq, double gamma_ineq, double *__restrict__ out) {
    const i64 inst = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (inst >= B) return;
    double r0 = 0.0, r1 = 0.0, r2 = -__builtin_inf(), c0 = 0.0, c1 = 0.0, c2 = -__builtin_inf();
    for (i64 g = 0; g < srows; ++g) {
        r0 += rp[(0 * srows + g) * Bp + inst];
        r1 += rp[(1 * srows + g) * Bp + inst];
        const double v = rp[(2 * srows + g) * Bp + inst];
        r2 = v > r2 ? v : r2;
    }
    for (i64 g = 0; g < scols; ++g) {
        c0 += cp[(0 * scols + g) * Bp + inst];
        c1 += cp[(1 * scols + g) * Bp + inst];
        const double v = cp[(2 * scols + g) * Bp + inst];
        c2 = v > c2 ? v : c2;
    }
    out[inst * 3 + 0] = c0 + 0.5 * gamma_eq * r0 + 0.5 * gamma_ineq * c1 + r1;  // :124-132
    out[inst * 3 + 1] = r2;                                                      // :221
    out[inst * 3 + 2] = (c2 > 0.0) ? c2 : 0.0;                                   // :222
}

// ---- set-up.  src [B x slen] row-major (or one shared [slen] vector) -> the tiled layout over len >= slen elements; elements
// slen .. len come from the shared `tail` (the slack part of a bound).  Padding instances: zero.
__global__ void k_admmb_scatter(i64 len, i64 slen, i64 B, int BT, i64 Bp, const double *__restrict__ src, int batched,
                                const double *__restrict__ tail, double *__restrict__ dst) {
    const i64 total = len * Bp;
    for (i64 o = (i64)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (i64)gridDim.x * blockDim.x) {
        const i64 k = o % BT, rest = o / BT, j = rest % len, tile = rest / len;
        const i64 inst = tile * BT + k;
        double v = 0.0;
        if (inst < B) v = j < slen ? src[batched ? inst * slen + j : j] : tail[j - slen];
        dst[o] = v;
    }
}

// the first `count` of len elements of every instance -> [B x count], row-major
__global__ void k_admmb_gather(i64 len, i64 count, i64 B, int BT, const double *__restrict__ src, double *__restrict__ dst) {
    const i64 total = count * B;
    for (i64 o = (i64)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (i64)gridDim.x * blockDim.x) {
        const i64 inst = o / count, j = o - inst * count;
        dst[o] = src[((inst / BT) * len + j) * BT + inst % BT];
    }
}

// q = (-c) + gamma_eq A^T b (k_admm_q; c = +0 on the slack columns), tiled
// (atb_batched: A^T b_k of instance k at atb + k * N, row-major, after slp_admm_batch_set_rhs)
__global__ void k_admmb_q(i64 N, i64 n, i64 B, int BT, i64 Bp, const double *__restrict__ c, const double *__restrict__ atb,
                          int atb_batched, double gamma_eq, double *__restrict__ q) {
    const i64 total = N * Bp;
    for (i64 o = (i64)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (i64)gridDim.x * blockDim.x) {
        const i64 k = o % BT, rest = o / BT, j = rest % N, tile = rest / N;
        const double cj = j < n ? c[(tile * n + j) * BT + k] : 0.0;
        const i64 inst = tile * BT + k;
        q[o] = inst < B ? (-cj) + gamma_eq * atb[atb_batched ? inst * N + j : j] : 0.0;
    }
}

// slp_admm_batch_set_rhs: `count` = rows * (1 or B) right-hand sides of the caller, row-major, brought to the state's units by
// the set-up chain's row scalings, one multiplication each in the chain's order (k_scale_vec: inf stays inf); row r of
// instance k goes to dst[k * dst_stride + r]
__global__ void k_admmb_scale_rhs(i64 rows, i64 count, const double *__restrict__ inv1, const double *__restrict__ inv2,
                                  const double *__restrict__ src, i64 dst_stride, double *__restrict__ dst) {
    for (i64 o = (i64)blockIdx.x * blockDim.x + threadIdx.x; o < count; o += (i64)gridDim.x * blockDim.x) {
        const i64 inst = o / rows, r = o - inst * rows;
        double v = inv1[r] * src[o];
        if (inv2) v = inv2[r] * v;
        dst[inst * dst_stride + r] = v;
    }
}

// slp_admm_batch_set_rhs: the slack part (columns n .. n + rows) of a tiled bound over N from src [B x rows] row-major (or one
// shared [rows] vector); the padding instances keep their zeros
__global__ void k_admmb_scatter_tail(i64 N, i64 n, i64 rows, i64 B, int BT, const double *__restrict__ src, int batched,
                                     double *__restrict__ dst) {
    const i64 total = rows * B;
    for (i64 o = (i64)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (i64)gridDim.x * blockDim.x) {
        const i64 inst = o / rows, r = o - inst * rows;
        dst[((inst / BT) * N + n + r) * BT + inst % BT] = src[batched ? o : r];
    }
}

// np.maximum(x, 0) (ADMM.py:98), element by element in whatever layout
__global__ void k_admmb_max0(i64 count, const double *__restrict__ x, double *__restrict__ xp) {
    for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (i64)gridDim.x * blockDim.x) xp[j] = (x[j] < 0.0) ? 0.0 : x[j];
}

}  // namespace slp

using namespace slp;

struct slp_admm_batch {
    slp_admm *base = nullptr;  // owned: the shared state (A, M's plan, A^T b, slack bounds)
    AdmmShared sh;
    i64 n = 0, N = 0, m = 0, B = 0, Bp = 0, ntiles = 0;
    int Bt = 1, form = 0;      // form: 0 tile, 1 levels
    i64 kmax = 1;              // iterations per launch of the tile form
    bool xp_is_x = false;      // false only before the first multiplier step (:98 vs :259)
    double gamma_eq = 2, gamma_ineq = 3;
    DevBuf<i64> lptr;
    DevBuf<double> c, q, lb, ub, x, xp0, y, lam, rowparts, colparts, out;
    bool lb_b = false, ub_b = false, x0_b = false;
    // slp_admm_batch_set_rhs: b tiled like lambda (b_b) or a shared vector of the state's own (b_own) in place of the set-up's;
    // lb_own / ub_own: a shared [N] bound of the state's own whose slack part was replaced (only while !lb_b / !ub_b)
    DevBuf<double> b;
    bool b_b = false, b_own = false, lb_own = false, ub_own = false;
    i64 iters = 0;             // whole iterations over the state's life: bumped where a multiplier half is enqueued
    bool mid = false;          // between sweep_step and multiplier_step
    // the stopping test (slp_admm_batch_set_stop); its buffers exist from the first arming on, and from then on the state
    // launches the STOP kernels.  Off while tol_residual < 0.
    bool armed = false;
    double tol_residual = -1.0, tol_step = 0.0;
    i64 check_every = 1;
    DevBuf<AdmmbCtl> ctl;      // per padded instance
    DevBuf<i32> running;       // the count of real instances that still run
    i64 stop_slices = 0;       // levels form: workgroups along x of its widest launch
    DevBuf<double> stopparts;  // levels form: 2 * stop_slices * Bp slots, the step's before the residual's
    ~slp_admm_batch() { if (base) slp_admm_destroy(base); }
};

namespace slp {

#define SLP_ADMMB_TILE(bt, CALL)                           \
    switch (bt) {                                          \
        case 1:  { constexpr int BT = 1;  CALL; } break;   \
        case 2:  { constexpr int BT = 2;  CALL; } break;   \
        case 4:  { constexpr int BT = 4;  CALL; } break;   \
        case 8:  { constexpr int BT = 8;  CALL; } break;   \
        case 16: { constexpr int BT = 16; CALL; } break;   \
        case 32: { constexpr int BT = 32; CALL; } break;   \
        default: { constexpr int BT = 64; CALL; } break;   \
    }

// Form and tile width: a function of the shapes and B only ("Batched ADMM").
//   tile form    when the levels are narrow (fewer than 4096 rows on average: even 16 instances per row do not fill the chip
//                from one level) or there are at least as many instances as compute units; width 1 while every instance can
//                have a compute unit of its own (B <= 256), then 4 (B <= 1024), then 16.
//   levels form  otherwise; width 1 for a single instance, 4 up to four, 16 beyond.
static void admmb_choose(i64 N, i64 nlevels, i64 B, int *form, int *bt) {
    const i64 mean_width = N / std::max<i64>(nlevels, 1);
    int f = (mean_width < 4096 || B >= 256) ? 0 : 1;
    if (const char *e = getenv("SLP_ADMM_BATCH_FORM")) {
        if (!strcmp(e, "tile")) f = 0;
        else if (!strcmp(e, "levels")) f = 1;
        else if (e[0]) throw Error(std::string("SLP_ADMM_BATCH_FORM must be tile or levels, not ") + e);
    }
    int w = f == 0 ? (B <= 256 ? 1 : (B <= 1024 ? 4 : 16)) : (B == 1 ? 1 : (B <= 4 ? 4 : 16));
    if (const char *e = getenv("SLP_ADMM_BATCH_TILE")) {
        const int v = atoi(e);
        if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16 || v == 32 || v == 64) w = v;
        else if (e[0]) throw Error(std::string("SLP_ADMM_BATCH_TILE must be a power of two up to 64, not ") + e);
    }
    *form = f;
    *bt = w;
}

static AdmmbArgs admmb_args(const slp_admm_batch *s) {
    AdmmbArgs a;
    const CsrDev &A = s->sh.a->a, &At = s->sh.a->at;
    a.N = s->N; a.m = s->m; a.n = s->n; a.B = s->B; a.nlevels = s->sh.nlevels;
    a.tptr = At.ptr.p; a.tidx = At.idx.p; a.tval = At.val.p;
    a.aptr = A.ptr.p; a.aidx = A.idx.p; a.aval = A.val.p;
    a.gptr = s->sh.gs_ptr; a.gidx = s->sh.gs_idx; a.gval = s->sh.gs_val; a.ginvd = s->sh.gs_invd; a.grows = s->sh.gs_rows;
    a.lptr = s->lptr.p;
    a.b = (s->b_b || s->b_own) ? s->b.p : s->sh.b;
    a.q = s->q.p; a.c = s->c.p;
    a.lb = (s->lb_b || s->lb_own) ? s->lb.p : s->sh.lb;
    a.ub = (s->ub_b || s->ub_own) ? s->ub.p : s->sh.ub;
    a.xp0 = s->xp0.p;
    a.x = s->x.p; a.y = s->y.p; a.lam = s->lam.p;
    a.lb_b = s->lb_b; a.ub_b = s->ub_b; a.xp0_b = s->x0_b; a.b_b = s->b_b;
    a.gamma_eq = s->gamma_eq; a.gamma_ineq = s->gamma_ineq;
    return a;
}

static dim3 admmb_grid(const slp_admm_batch *s, i64 rows) { return dim3((unsigned)grid_for(rows * s->Bt, kBlock), (unsigned)s->ntiles); }

// what a launch of a STOP kernel is told: the count so far, and the cadence only where the test is to be evaluated
static AdmmbStop admmb_stop(const slp_admm_batch *s, bool test) {
    AdmmbStop sp;
    sp.ctl = s->ctl.p;
    sp.running = s->running.p;
    sp.t0 = s->iters;
    sp.check_every = (test && s->tol_residual >= 0.0) ? s->check_every : 0;
    sp.tol_residual = s->tol_residual;
    sp.tol_step = s->tol_step;
    return sp;
}

template <bool STOP>
static void admmb_run_tile(slp_admm_batch *s, const AdmmbArgs &a, i64 iters, int stages, bool test) {
    while (iters > 0) {
        const i64 k = std::min(iters, s->kmax);
        const int first = ((stages & 1) && !s->xp_is_x) ? 1 : 0;
        if (s->b_b) {
            SLP_ADMMB_TILE(s->Bt, hipLaunchKernelGGL((k_admmb_tile<BT, STOP, true>), dim3((unsigned)s->ntiles), dim3(kAdmmbBlock), 0, ctx().stream,
                                                     a, (int)k, first, stages, admmb_stop(s, test)));
        } else {
            SLP_ADMMB_TILE(s->Bt, hipLaunchKernelGGL((k_admmb_tile<BT, STOP, false>), dim3((unsigned)s->ntiles), dim3(kAdmmbBlock), 0, ctx().stream,
                                                     a, (int)k, first, stages, admmb_stop(s, test)));
        }
        SLP_HIP(hipGetLastError());
        if (stages & 2) {
            s->xp_is_x = true;  // :259
            s->iters += k;
        }
        iters -= k;
    }
}

template <bool STOP>
static void admmb_run_levels(slp_admm_batch *s, const AdmmbArgs &a, i64 iters, int stages, bool test) {
    hipStream_t st = ctx().stream;
    const AdmmbCtl *ctl = s->ctl.p;
    double *steps = s->stopparts.p, *residuals = s->stopparts.p + s->stop_slices * s->Bp;
    for (i64 it = 0; it < iters; ++it) {
        AdmmbStop sp = admmb_stop(s, test);
        sp.t0 = s->iters + 1;  // the iteration these launches belong to
        const bool check = STOP && sp.check_every > 0 && sp.t0 % sp.check_every == 0;
        i64 nstep = 0, nres = 0;
        if (stages & 1) {
            if (check) SLP_HIP(hipMemsetAsync(steps, 0, (size_t)(s->stop_slices * s->Bp) * sizeof(double), st));
            SLP_ADMMB_TILE(s->Bt, hipLaunchKernelGGL((k_admmb_rhs<BT, STOP>), admmb_grid(s, s->N), dim3(kBlock), 0, st, a, s->xp_is_x ? 0 : 1,
                                                     ctl));
            for (i64 l = 0; l < s->sh.nlevels; ++l) {
                const i64 beg = s->sh.lptr[(size_t)l], end = s->sh.lptr[(size_t)l + 1];
                if (end <= beg) continue;
                const dim3 grid = admmb_grid(s, end - beg);
                nstep = std::max<i64>(nstep, grid.x);
                SLP_ADMMB_TILE(s->Bt, hipLaunchKernelGGL((k_admmb_level<BT, STOP>), grid, dim3(kBlock), 0, st, a, beg, end, ctl, s->Bp,
                                                         check ? steps : nullptr));
            }
        }
        if (stages & 2) {
            s->xp_is_x = true;
            ++s->iters;
            if (s->m > 0) {
                const dim3 grid = admmb_grid(s, s->m);
                nres = grid.x;
                if (s->b_b) {
                    SLP_ADMMB_TILE(s->Bt, hipLaunchKernelGGL((k_admmb_mult<BT, STOP, true>), grid, dim3(kBlock), 0, st, a, ctl, s->Bp,
                                                             check ? residuals : nullptr));
                } else {
                    SLP_ADMMB_TILE(s->Bt, hipLaunchKernelGGL((k_admmb_mult<BT, STOP, false>), grid, dim3(kBlock), 0, st, a, ctl, s->Bp,
                                                             check ? residuals : nullptr));
                }
            }
        }
        if (check) {
            SLP_REQUIRE(nstep <= s->stop_slices && nres <= s->stop_slices, "slp_admm_batch: the stopping test's slots are too few");
            hipLaunchKernelGGL(k_admmb_decide, dim3((unsigned)s->B), dim3(kBlock), 0, st, s->Bp, nstep, steps, nres, residuals, stages, sp);
        }
        SLP_HIP(hipGetLastError());
    }
}

// stages: bit 0 right-hand side + sweep, bit 1 multiplier; `iters` whole iterations when both are set.  test: evaluate the
// stopping test where it is armed (not in slp_admm_batch_bench).  An armed state asks once per call that ends iterations
// whether anything is left to run.
static void admmb_run(slp_admm_batch *s, i64 iters, int stages, bool test = true) {
    if (stages & 2) s->mid = false;
    else s->mid = true;
    if (s->N == 0 || iters <= 0) return;
    if (s->armed && test && (stages & 2)) {
        i32 running = 0;
        s->running.download(&running, 1);
        if (running == 0) return;
    }
    const AdmmbArgs a = admmb_args(s);
    if (s->form == 0) s->armed ? admmb_run_tile<true>(s, a, iters, stages, test) : admmb_run_tile<false>(s, a, iters, stages, test);
    else s->armed ? admmb_run_levels<true>(s, a, iters, stages, test) : admmb_run_levels<false>(s, a, iters, stages, test);
}

static dim3 admmb_report_grid(const slp_admm_batch *s, i64 rows) {
    const i64 per_block = kBlock / s->Bt;
    i64 g = (rows + per_block - 1) / per_block;
    const i64 cap = std::max<i64>(1, kAdmmbMaxSlices / per_block);
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return dim3((unsigned)g, (unsigned)s->ntiles);
}

static void admmb_scatter(slp_admm_batch *s, i64 len, i64 slen, const double *src, int batched, const double *tail, double *dst) {
    hipLaunchKernelGGL(k_admmb_scatter, dim3(grid_for(len * s->Bp, kBlock)), dim3(kBlock), 0, ctx().stream, len, slen, s->B, s->Bt, s->Bp, src,
                       batched, tail, dst);
    SLP_HIP(hipGetLastError());
}

static void admmb_download(slp_admm_batch *s, const DevBuf<double> &src, i64 len, i64 count, double *host) {
    if (count == 0) return;
    DevBuf<double> stage((size_t)count * (size_t)s->B);
    hipLaunchKernelGGL(k_admmb_gather, dim3(grid_for(count * s->B, kBlock)), dim3(kBlock), 0, ctx().stream, len, count, s->B, s->Bt, src.p,
                       stage.p);
    SLP_HIP(hipGetLastError());
    stage.download(host, (size_t)count * (size_t)s->B);
}

static void admmb_check_indices(const char *what, i64 rows, i64 n, const int64_t *indptr, const int32_t *indices) {
    SLP_REQUIRE(indptr[0] == 0 && indptr[rows] >= 0, std::string("slp_admm_batch_create_lp: bad row pointer of the ") + what + " block");
    for (i64 q = 0; q < indptr[rows]; ++q)
        SLP_REQUIRE(indices[q] >= 0 && indices[q] < n, std::string("slp_admm_batch_create_lp: column index out of range in the ") + what + " block");
}

}  // namespace slp

extern "C" {

slp_admm_batch *slp_admm_batch_create_lp(int64_t n, int64_t m_eq, const int64_t *eq_indptr, const int32_t *eq_indices,
                                         const double *eq_data, const double *b_eq, int64_t m_ineq, const int64_t *in_indptr,
                                         const int32_t *in_indices, const double *in_data, const double *b_lower,
                                         const double *b_upper, int64_t batch, const double *c, int c_batched, const double *lb,
                                         int lb_batched, const double *ub, int ub_batched, const double *x0, int x0_batched,
                                         double gamma_eq, double gamma_ineq, int use_preconditioning) {
    SLP_API_PTR({
        SLP_REQUIRE(batch >= 1, "slp_admm_batch_create_lp: batch must be at least 1");
        SLP_REQUIRE(in_indptr, "slp_admm_batch_create_lp: the inequality block is required (the reference's standard form is "
                               "undefined without it, tools.py:92)");
        SLP_REQUIRE(n >= 1 && m_eq >= 0 && m_ineq >= 0 && c && lb && ub, "slp_admm_batch_create_lp: bad arguments");
        SLP_REQUIRE(m_eq == 0 || (eq_indptr && b_eq), "slp_admm_batch_create_lp: NULL equality block");
        SLP_REQUIRE(c_batched || batch == 1, "slp_admm_batch_create_lp: c must be [batch x n] (c_batched = 1) for more than one instance");
        if (eq_indptr) admmb_check_indices("equality", m_eq, n, eq_indptr, eq_indices);
        admmb_check_indices("inequality", m_ineq, n, in_indptr, in_indices);
        const i64 N = n + m_ineq, m = m_eq + m_ineq;
        // M's level count is not known yet: the form's rule needs it, so the width used for the estimate is the widest padding
        // either form can choose for this B (at most 15 padding instances)
        const double bp_max = (double)((batch + 15) / 16 * 16);
        {
            // nothing is allocated, and no batched argument is read, before this check.  Batched: x, y, q over N, lambda over m, c
            // over n, xp0 / lb / ub over N where they differ per instance; the staging of one host argument and of the starts; the
            // report's slice sums.  Shared: both copies of A, M with its level-ordered copy and the lane records of the set-up
            // (at most sum of squared row lengths entries).
            i64 free_b = 0, total_b = 0;
            SLP_REQUIRE(slp_device_memory(&free_b, &total_b) == 0, slp_last_error());
            const double vectors = ((3.0 + (x0_batched ? 1 : 0) + (lb_batched ? 1 : 0) + (ub_batched ? 1 : 0)) * (double)N + (double)m + (double)n) *
                                   8.0 * bp_max;
            double nnz_a = (double)in_indptr[m_ineq] + (double)m_ineq + (eq_indptr ? (double)eq_indptr[m_eq] : 0.0), sq = 0.0;
            for (i64 i = 0; i < m_ineq; ++i) { const double l = (double)(in_indptr[i + 1] - in_indptr[i]) + 1.0; sq += l * l; }
            for (i64 i = 0; eq_indptr && i < m_eq; ++i) { const double l = (double)(eq_indptr[i + 1] - eq_indptr[i]); sq += l * l; }
            const double need = vectors + 8.0 * (double)(x0_batched ? N + n : n) * (double)batch + 8.0 * 6.0 * kAdmmbMaxSlices * bp_max +
                                64.0 * nnz_a + 40.0 * (sq + (double)N) + 16.0 * 8.0 * (double)(N + m);
            const double have = (double)free_b + (double)slp_cached_bytes();
            if (need > have)
                throw Error("slp_admm_batch_create_lp: " + std::to_string(batch) + " instances need " + std::to_string(need / 1e9) +
                            " GB of device memory (batched vectors: " + std::to_string(vectors / 1e9) + " GB), " +
                            std::to_string(have / 1e9) + " GB are free");
        }
        auto *s = new slp_admm_batch();
        slp_matrix *ai2 = nullptr;
        try {
            hipStream_t st = ctx().stream;
            // instance 0's vectors stand for the shared chain: nothing of it but q, the start and the bounds of the original
            // variables depends on them, and those are rebuilt per instance below
            s->base = admm_create_lp(n, m_eq, eq_indptr, eq_indices, eq_data, b_eq, m_ineq, in_indptr, in_indices, in_data, b_lower, b_upper, c,
                                     lb, ub, x0, gamma_eq, gamma_ineq, use_preconditioning, SLP_ORDER_SEQUENTIAL, x0_batched ? &ai2 : nullptr, true);
            admm_shared(s->base, &s->sh);
            require_csr(s->sh.a, "slp_admm_batch_create_lp");
            s->n = n; s->N = N; s->m = m; s->B = batch;
            s->gamma_eq = gamma_eq; s->gamma_ineq = gamma_ineq;
            admmb_choose(N, s->sh.nlevels, batch, &s->form, &s->Bt);
            s->ntiles = (batch - 1) / s->Bt + 1;
            s->Bp = s->ntiles * s->Bt;
            SLP_REQUIRE(s->form == 0 || s->ntiles <= 65535, "slp_admm_batch_create_lp: at most 65535 tiles in the levels form");
            {
                i64 units = (N * s->Bt + kAdmmbBlock - 1) / kAdmmbBlock + (m * s->Bt + kAdmmbBlock - 1) / kAdmmbBlock;
                for (i64 l = 0; l < s->sh.nlevels; ++l)
                    units += std::max<i64>(1, ((s->sh.lptr[(size_t)l + 1] - s->sh.lptr[(size_t)l]) * s->Bt + kAdmmbBlock - 1) / kAdmmbBlock);
                s->kmax = std::min<i64>(64, std::max<i64>(1, kAdmmbUnitsPerLaunch / std::max<i64>(units, 1)));
            }
            s->lb_b = lb_batched != 0; s->ub_b = ub_batched != 0; s->x0_b = x0 && x0_batched;
            s->lptr.upload(s->sh.lptr.data(), s->sh.lptr.size());
            const size_t nb = (size_t)N * (size_t)s->Bp;
            s->c.alloc((size_t)n * (size_t)s->Bp);
            s->q.alloc(nb); s->x.alloc(nb); s->y.alloc(nb);
            s->y.zero();
            s->lam.alloc((size_t)m * (size_t)s->Bp);
            s->lam.zero();
            s->rowparts.alloc((size_t)3 * kAdmmbMaxSlices * (size_t)s->Bp);
            s->colparts.alloc((size_t)3 * kAdmmbMaxSlices * (size_t)s->Bp);
            s->out.alloc((size_t)3 * (size_t)s->Bp);
            s->out.zero();
            {
                DevBuf<double> stage((size_t)n * (size_t)batch);
                auto stage_in = [&](const double *host, int batched) {
                    SLP_HIP(hipMemcpyAsync(stage.p, host, (size_t)n * (size_t)(batched ? batch : 1) * sizeof(double), hipMemcpyHostToDevice, st));
                };
                stage_in(c, c_batched);
                admmb_scatter(s, n, n, stage.p, c_batched, nullptr, s->c.p);
                // A^T b of the set-up has not been overwritten: the base state never iterates
                hipLaunchKernelGGL(k_admmb_q, dim3(grid_for(N * s->Bp, kBlock)), dim3(kBlock), 0, st, N, n, s->B, s->Bt, s->Bp, s->c.p, s->sh.atb,
                                   0, gamma_eq, s->q.p);
                SLP_HIP(hipGetLastError());
                SLP_HIP(hipStreamSynchronize(st));  // the stage is reused
                if (s->lb_b) {   // [lb_k; scaled b_lower]
                    s->lb.alloc(nb);
                    stage_in(lb, 1);
                    admmb_scatter(s, N, n, stage.p, 1, s->sh.lb + n, s->lb.p);
                    SLP_HIP(hipStreamSynchronize(st));
                }
                if (s->ub_b) {
                    s->ub.alloc(nb);
                    stage_in(ub, 1);
                    admmb_scatter(s, N, n, stage.p, 1, s->sh.ub + n, s->ub.p);
                    SLP_HIP(hipStreamSynchronize(st));
                }
                if (s->x0_b) {   // x_k = [x0_k; A_ineq x0_k] with the scaled block, in its stored order (:84-86)
                    DevBuf<double> starts((size_t)N * (size_t)batch);
                    stage_in(x0, 1);
                    for (i64 k = 0; k < batch; ++k) {
                        SLP_HIP(hipMemcpyAsync(starts.p + k * N, stage.p + k * n, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
                        if (m_ineq) launch_spmv(ai2->a, starts.p + k * N, starts.p + k * N + n, SLP_ORDER_SEQUENTIAL);
                    }
                    admmb_scatter(s, N, N, starts.p, 1, nullptr, s->x.p);
                    s->xp0.alloc(nb);
                    hipLaunchKernelGGL(k_admmb_max0, dim3(grid_for((i64)nb, kBlock)), dim3(kBlock), 0, st, (i64)nb, s->x.p, s->xp0.p);
                    SLP_HIP(hipGetLastError());
                    SLP_HIP(hipStreamSynchronize(st));
                } else {         // one start for all: held once
                    admmb_scatter(s, N, N, s->sh.x0, 0, nullptr, s->x.p);
                    s->xp0.alloc((size_t)N);
                    hipLaunchKernelGGL(k_admmb_max0, dim3(grid_for(N, kBlock)), dim3(kBlock), 0, st, N, s->sh.x0, s->xp0.p);
                    SLP_HIP(hipGetLastError());
                }
            }
            SLP_HIP(hipStreamSynchronize(st));
            delete ai2;
            ai2 = nullptr;
        } catch (...) {
            delete ai2;
            delete s;
            throw;
        }
        return s;
    })
}

void slp_admm_batch_destroy(slp_admm_batch *s) { delete s; }

int slp_admm_batch_iterate(slp_admm_batch *s, int64_t k) {
    SLP_API_INT({ SLP_REQUIRE(s && k >= 0, "slp_admm_batch_iterate: bad arguments"); admmb_run(s, k, 3); })
}

int slp_admm_batch_sweep_step(slp_admm_batch *s) { SLP_API_INT({ SLP_REQUIRE(s, "NULL handle"); admmb_run(s, 1, 1); }) }

int slp_admm_batch_multiplier_step(slp_admm_batch *s) { SLP_API_INT({ SLP_REQUIRE(s, "NULL handle"); admmb_run(s, 1, 2); }) }

int slp_admm_batch_report(slp_admm_batch *s, double *out) {
    SLP_API_INT({
        SLP_REQUIRE(s && out, "slp_admm_batch_report: NULL argument");
        hipStream_t st = ctx().stream;
        const AdmmbArgs a = admmb_args(s);
        const dim3 gr = admmb_report_grid(s, s->m), gc = admmb_report_grid(s, s->N);
        const i64 srows = (i64)gr.x * kBlock / s->Bt, scols = (i64)gc.x * kBlock / s->Bt;
        SLP_ADMMB_TILE(s->Bt, hipLaunchKernelGGL((k_admmb_report_cols<BT>), gc, dim3(kBlock), 0, st, a, s->xp_is_x ? 0 : 1, s->Bp, s->colparts.p));
        SLP_HIP(hipGetLastError());
        SLP_ADMMB_TILE(s->Bt, hipLaunchKernelGGL((k_admmb_report_rows<BT>), gr, dim3(kBlock), 0, st, a, s->Bp, s->rowparts.p));
        SLP_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_admmb_report_final, dim3((unsigned)((s->B + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, s->B, s->Bp, srows,
                           s->rowparts.p, scols, s->colparts.p, s->gamma_eq, s->gamma_ineq, s->out.p);
        SLP_HIP(hipGetLastError());
        s->out.download(out, (size_t)3 * (size_t)s->B);
    })
}

int slp_admm_batch_get_x(slp_admm_batch *s, double *x, int64_t count) {
    SLP_API_INT({
        SLP_REQUIRE(s && x && count >= 0 && count <= s->N, "slp_admm_batch_get_x: bad arguments");
        admmb_download(s, s->x, s->N, count, x);
    })
}

int slp_admm_batch_get_lambda(slp_admm_batch *s, double *lam) {
    SLP_API_INT({ SLP_REQUIRE(s && lam, "NULL argument"); admmb_download(s, s->lam, s->m, s->m, lam); })
}

int64_t slp_admm_batch_num_levels(const slp_admm_batch *s) { return s ? s->sh.nlevels : -1; }

int slp_admm_batch_form(const slp_admm_batch *s) { return s ? s->form : -1; }

int slp_admm_batch_bench(slp_admm_batch *s, int64_t k, double *ms) {
    SLP_API_INT({
        SLP_REQUIRE(s && k > 0 && ms, "slp_admm_batch_bench: bad arguments");
        Context &c = ctx();
        SLP_HIP(hipEventRecord(c.ev0, c.stream));
        admmb_run(s, k, 3, false);
        SLP_HIP(hipEventRecord(c.ev1, c.stream));
        SLP_HIP(hipEventSynchronize(c.ev1));
        float f = 0.f;
        SLP_HIP(hipEventElapsedTime(&f, c.ev0, c.ev1));
        *ms = (double)f / (double)k;
    })
}

int slp_admm_batch_set_rhs(slp_admm_batch *s, const double *b_eq, int b_eq_batched, const double *b_lower, int b_lower_batched,
                           const double *b_upper, int b_upper_batched) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_admm_batch_set_rhs: NULL handle");
        SLP_REQUIRE(s->iters == 0 && !s->mid && !s->xp_is_x,
                    "slp_admm_batch_set_rhs: the state has iterated; the right-hand sides are set before the first iteration or half iteration");
        hipStream_t st = ctx().stream;
        const i64 N = s->N, n = s->n, m = s->m, m_eq = s->sh.m_eq, m_ineq = N - n, B = s->B;
        SLP_REQUIRE(m_eq + m_ineq == m, "slp_admm_batch_set_rhs: the state does not know its blocks");
        if (m_eq == 0) b_eq = nullptr;       // no equality rows: nothing to replace
        if (m_ineq == 0) b_lower = b_upper = nullptr;
        SLP_REQUIRE(!b_eq || s->sh.scale_eq, "slp_admm_batch_set_rhs: the state did not keep the row scaling of the equality block");
        SLP_REQUIRE(!(b_lower || b_upper) || s->sh.scale_ineq,
                    "slp_admm_batch_set_rhs: the state did not keep the row scaling of the inequality block");
        const bool eq_b = b_eq && b_eq_batched, lo_b = b_lower && b_lower_batched, hi_b = b_upper && b_upper_batched;
        const size_t nb = (size_t)N * (size_t)s->Bp, mb = (size_t)m * (size_t)s->Bp;
        const bool new_b = eq_b && !s->b_b, new_lb = lo_b && !s->lb_b, new_ub = hi_b && !s->ub_b;
        SLP_HIP(hipStreamSynchronize(st));
        {
            // nothing is allocated before this check: what stays (the tiled b, the bounds that become batched, a shared vector of
            // the state's own) and the staging of this call (the caller's rows, [b_k; 0] and A^T b_k per instance)
            i64 free_b = 0, total_b = 0;
            SLP_REQUIRE(slp_device_memory(&free_b, &total_b) == 0, slp_last_error());
            double need = 8.0 * ((new_b ? (double)mb : 0.0) + ((new_lb ? 1.0 : 0.0) + (new_ub ? 1.0 : 0.0)) * (double)nb);
            if (b_eq) need += 8.0 * (double)(eq_b ? B : 1) * (double)(m_eq + m + N) + 8.0 * (double)m;
            if (b_lower || b_upper) need += 8.0 * 2.0 * (double)((lo_b || hi_b) ? B : 1) * (double)m_ineq + 8.0 * 2.0 * (double)N;
            const double have = (double)free_b + (double)slp_cached_bytes();
            if (need > have)
                throw Error("slp_admm_batch_set_rhs: the right-hand sides of " + std::to_string(B) + " instances need " +
                            std::to_string(need / 1e9) + " GB of device memory, " + std::to_string(have / 1e9) + " GB are free");
        }
        if (b_eq) {
            const i64 reps = eq_b ? B : 1;
            DevBuf<double> stage((size_t)(reps * m_eq)), bk((size_t)(reps * m)), atb((size_t)(reps * N));
            stage.upload(b_eq, (size_t)(reps * m_eq));
            bk.zero();   // the inequality rows of b are 0 (tools.py:88-127)
            hipLaunchKernelGGL(k_admmb_scale_rhs, dim3(grid_for(reps * m_eq, kBlock)), dim3(kBlock), 0, st, m_eq, reps * m_eq, s->sh.scale_eq,
                               s->sh.scale_rows, stage.p, m, bk.p);
            SLP_HIP(hipGetLastError());
            // A^T b_k with the set-up's product (ADMM.py:95), then q_k
            for (i64 k = 0; k < reps; ++k) launch_spmv(s->sh.a->at, bk.p + k * m, atb.p + k * N, SLP_ORDER_SEQUENTIAL);
            hipLaunchKernelGGL(k_admmb_q, dim3(grid_for(N * s->Bp, kBlock)), dim3(kBlock), 0, st, N, n, s->B, s->Bt, s->Bp, s->c.p, atb.p,
                               eq_b ? 1 : 0, s->gamma_eq, s->q.p);
            SLP_HIP(hipGetLastError());
            if (eq_b || s->b_b) {
                if (!s->b_b) s->b.alloc(mb);
                admmb_scatter(s, m, m, bk.p, eq_b ? 1 : 0, nullptr, s->b.p);
                s->b_b = true;
                s->b_own = false;
            } else {
                if (!s->b_own) s->b.alloc((size_t)m);
                SLP_HIP(hipMemcpyAsync(s->b.p, bk.p, (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, st));
                s->b_own = true;
            }
            SLP_HIP(hipStreamSynchronize(st));   // the staging goes away
        }
        // the slack part of a bound: the scaled b_lower / b_upper (:76-83; -inf / +inf stay)
        auto slack = [&](const double *host, bool batched, DevBuf<double> &bound, bool &bound_b, bool &bound_own, const double *shared) {
            const i64 reps = batched ? B : 1;
            DevBuf<double> stage((size_t)(reps * m_ineq)), scaled((size_t)(reps * m_ineq));
            stage.upload(host, (size_t)(reps * m_ineq));
            hipLaunchKernelGGL(k_admmb_scale_rhs, dim3(grid_for(reps * m_ineq, kBlock)), dim3(kBlock), 0, st, m_ineq, reps * m_ineq,
                               s->sh.scale_ineq, (const double *)nullptr, stage.p, m_ineq, scaled.p);
            SLP_HIP(hipGetLastError());
            if (batched && !bound_b) {   // the bound becomes batched over N because of its slack part
                const double *cur = bound_own ? bound.p : shared;
                DevBuf<double> tiled(nb);
                admmb_scatter(s, N, n, cur, 0, cur + n, tiled.p);
                SLP_HIP(hipStreamSynchronize(st));
                bound = std::move(tiled);
                bound_b = true;
                bound_own = false;
            }
            if (bound_b) {
                hipLaunchKernelGGL(k_admmb_scatter_tail, dim3(grid_for(m_ineq * B, kBlock)), dim3(kBlock), 0, st, N, n, m_ineq, B, s->Bt, scaled.p,
                                   batched ? 1 : 0, bound.p);
                SLP_HIP(hipGetLastError());
            } else {
                if (!bound_own) {
                    bound.alloc((size_t)N);
                    SLP_HIP(hipMemcpyAsync(bound.p, shared, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
                    bound_own = true;
                }
                SLP_HIP(hipMemcpyAsync(bound.p + n, scaled.p, (size_t)m_ineq * sizeof(double), hipMemcpyDeviceToDevice, st));
            }
            SLP_HIP(hipStreamSynchronize(st));
        };
        if (b_lower) slack(b_lower, lo_b, s->lb, s->lb_b, s->lb_own, s->sh.lb);
        if (b_upper) slack(b_upper, hi_b, s->ub, s->ub_b, s->ub_own, s->sh.ub);
    })
}

int slp_admm_batch_set_stop(slp_admm_batch *s, double tol_residual, double tol_step, int64_t check_every) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_admm_batch_set_stop: NULL handle");
        SLP_REQUIRE(tol_residual < 0.0 || (std::isfinite(tol_residual) && std::isfinite(tol_step) && tol_step >= 0.0 && check_every >= 1),
                    "slp_admm_batch_set_stop: tol_residual and tol_step must be finite and >= 0 with check_every >= 1 (tol_residual < 0 "
                    "turns the test off)");
        SLP_REQUIRE(!s->mid, "slp_admm_batch_set_stop: called between sweep_step and multiplier_step (whole iterations only)");
        if (tol_residual >= 0.0 && !s->armed) {  // the first arming: records (padding instances stopped), the count, the slots
            const size_t bp = (size_t)s->Bp;
            std::vector<AdmmbCtl> ctl(bp);
            for (size_t k = 0; k < bp; ++k) ctl[k] = AdmmbCtl{0, k < (size_t)s->B ? 0 : 1, 0, __builtin_inf(), __builtin_inf(), 0.0};
            const i32 running = (i32)std::min<i64>(s->B, 0x7fffffff);
            if (s->form == 1) {
                i64 slices = admmb_grid(s, s->m).x;
                for (i64 l = 0; l < s->sh.nlevels; ++l)
                    slices = std::max<i64>(slices, admmb_grid(s, s->sh.lptr[(size_t)l + 1] - s->sh.lptr[(size_t)l]).x);
                s->stop_slices = slices;
                s->stopparts.alloc((size_t)2 * (size_t)slices * bp);
            }
            s->ctl.upload(ctl.data(), bp);
            s->running.upload(&running, 1);
            s->armed = true;
        }
        s->tol_residual = tol_residual < 0.0 ? -1.0 : tol_residual;
        if (tol_residual >= 0.0) {
            s->tol_step = tol_step;
            s->check_every = check_every;
        }
        SLP_HIP(hipStreamSynchronize(ctx().stream));
    })
}

int slp_admm_batch_stop_state(slp_admm_batch *s, int64_t *iterations, int32_t *stopped, double *residual, double *step) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_admm_batch_stop_state: NULL handle");
        const size_t count = (size_t)s->B;
        std::vector<AdmmbCtl> ctl(count, AdmmbCtl{0, 0, 0, __builtin_inf(), __builtin_inf(), 0.0});
        if (s->armed) s->ctl.download(ctl.data(), count);
        else SLP_HIP(hipStreamSynchronize(ctx().stream));
        for (size_t k = 0; k < count; ++k) {
            if (iterations) iterations[k] = ctl[k].stopped ? ctl[k].stop_iter : s->iters;
            if (stopped) stopped[k] = ctl[k].stopped;
            if (residual) residual[k] = ctl[k].residual;
            if (step) step[k] = ctl[k].step;
        }
    })
}

}  // extern "C"
