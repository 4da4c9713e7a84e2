// slp_dga_batch.hip -- batched dual gradient ascent: B LPs over ONE constraint matrix K = [A_eq; A_ineq] and one right-hand side
// advance per launch.  No counterpart in the reference (B solves are B calls of dual_gradient_ascent, DualGradientAscent.py:68-245).
// The instances differ in c and, optionally, in lb, ub and the start multipliers.  Every chain of additions is the single
// solver's (slp_dga_shared.h, included by slp_dga.hip too), so instance k is bit for bit what slp_dga computes on its data:
// x, y, the tie draws taken and the status flags, on either search path, for any B and any split of the iterations over calls.
// slp_batch_dga_set_rhs (include/slp_hip_ext_batch_rhs.h), before the first iteration, gives every instance a right-hand side of its
// own: b then holds B segments of m and its readers -- the gradient pass, the y . b of the bound and of the report -- take
// b + instance * b_stride (0 for the shared vector of the constructor).
//
// Layout: instance-major.  A batched vector over the n variables (c, x, c_bar, d; lb, ub when they are per instance) is B
// segments of n, over the m rows (y, K x, g) B segments of m; the sort keys, sorted columns and both scan outputs are B segments
// of n, which is what the segmented sort needs.  A launch is a grid of (the single solver's blocks, B): blockIdx.y is the
// instance, and the kernel body runs on that instance's segments exactly as the single solver's kernel runs on its vectors.
// One DgaCtl per instance carries the step, g.b, the min ratio, the draws consumed, `active`, nb, the sticky flags and `frozen`.
// Nothing is read back inside slp_batch_dga_iterate (with a stopping test: the controls once, before its first launch).
//
// One iteration = column pass (both partial sums of K^T y, c_bar and the dual argmin, fused), row pass (K x), then per block of
// rows: gradient pass with its 256 partial results, the block's scalars, d = K^T g, the search, the update.  The search is
//   fused   -- n <= 8192: one workgroup of 1024 threads per instance runs the single solver's LDS search (grid = B);
//   general -- keys of all (instance, column), a stable sort of the B segments, tile sums / tile offsets / final scans over
//              (tiles, B), one wave per instance for the bisection.  The sort: ONE segmented radix sort (the segment of an instance
//              whose block predicate is off is empty; a workgroup per segment, slow on long segments) or a device-wide stable
//              sort of all keys followed by a stable sort by instance (the same order; the default above 2048 variables).
// Tie draws: every solve reads the SAME stream of uniform draws, each instance at its own position ctl[k].consumed; the device
// holds the window min(consumed) .. of that stream and the host keeps it two draws per iteration ahead of max(consumed).
// An instance whose start has dual energy -inf (what makes the single solve return at once, :133-139) is frozen: its x stays the
// start's dual argmin, its y the start, and the others go on.
//
// Stopping per instance (slp_batch_dga_set_stop, include/slp_hip_ext_dga_batch.h; off after create).  Iterations t count from 1
// over the life of the state.  At the end of an iteration t with t % check_every == 0 -- the host knows them from `iters`, the
// iterations in between are launched as without the test -- every instance that is neither frozen nor stopped evaluates
//   step_t  = max |y_t - y_{t-1}| over its m multipliers, as np.max (a NaN stays), the inequality part after its clamp, 0 from a
//             kind of rows whose block predicate was off: the update pass of a check iteration (k_dgab_update_step) reduces it
//             per workgroup, with ordinary stores into slots of its own, for both blocks of rows;
//   bound_t = the dual energy of y_t, only when cut-offs were given: one column pass over the live instances into the report's
//             buffers (the instance's own x and c_bar stay), then the report's two reductions without the K x product and the
//             violations (dga_energy_x_body, the y . b chain of dga_energy_y_body<false>) and, by one lane, the report's
//             sequential sum of the 256 partial results (dga_bound_finish): bit for bit column 0 of slp_batch_dga_report;
// and stops iff step_t <= tol (tol >= 0) or bound_t >= targets[k] (targets[k] < +inf) -- never on a NaN, nor while its sticky
// DGA_NAN bit is up.  k_dgab_decide, one workgroup per instance, folds the slots, writes the instance's record (DgabStop, an
// array of its own beside DgaCtl, whose layout the single and the list solver share: stopping iteration, reason, last evaluated
// step and bound) and retires the instance by the second non-zero value of DgaCtl::frozen, kDgaStopped: every kernel here
// tests that field for truth, so a stopped instance runs no column or row pass, has an empty sort segment, does no search and no
// update, and the hot kernels are those of the state without a test.  slp_batch_dga_frozen reports the value 1 only.  A stopped
// instance keeps y_t, the x and c_bar of the top of iteration t, its draws taken and its flags.  It is no reader of the stream of
// draws any more (slp_dga_draws.h), so it cannot be resumed: no call clears the mark.  On a state that was ever armed
// slp_batch_dga_iterate first reads the controls (one synchronising read) and launches nothing, leaving `iters`, when no instance
// moves; nothing else is read back, so a stopping iteration does not depend on how a run is split into calls.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "slp_common.h"
#include "slp_kernels.h"
#include "slp_many.h"
#include "slp_dga_shared.h"
#include "../../include/slp_hip_ext_dga_batch.h"
#include "../../include/slp_hip_ext_batch_rhs.h"

using namespace slp;

namespace {

// the stopping test's record of an instance
struct DgabStop {
    i64 done;       // its stopping iteration, 0 while it is not stopped
    double step;    // the last evaluated max |y_t - y_{t-1}|, +inf before the first test
    double bound;   // the last evaluated dual energy, -inf before the first
    i32 reason, pad;   // bit 0: the step met tol, bit 1: the bound met the cut-off; 0 while it is not stopped
};

// column pass: one lane per (column j, instance): the two masked sums of K^T y in storage order (the single solver's two
// SEQUENTIAL products over y with the other kind of rows set to 0.0), c_bar = (c + s_eq) + s_ineq, x = the dual argmin
__global__ __launch_bounds__(kBlock) void k_dgab_cols(i64 n, i64 m, i64 m_eq, const i64 *__restrict__ tptr, const i32 *__restrict__ tidx,
                                                      const double *__restrict__ tval, const double *__restrict__ y,
                                                      const double *__restrict__ c, const double *__restrict__ lb, i64 lb_stride,
                                                      const double *__restrict__ ub, i64 ub_stride, const DgaCtl *__restrict__ ctl,
                                                      int skip_frozen, double *__restrict__ cbar, double *__restrict__ x) {
    const i64 inst = blockIdx.y;
    if (skip_frozen && ctl[inst].frozen) return;
    const double *__restrict__ yk = y + inst * m;
    for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (i64)gridDim.x * blockDim.x) {
        double se = 0.0, si = 0.0;
        for (i64 q = tptr[j]; q < tptr[j + 1]; ++q) {
            const i32 r = tidx[q];
            const double a = tval[q], yv = yk[r];
            se += a * (r < m_eq ? yv : 0.0);
            si += a * (r < m_eq ? 0.0 : yv);
        }
        double cb = c[inst * n + j];
        if (m_eq > 0) cb = cb + se;
        if (m_eq < m) cb = cb + si;
        cbar[inst * n + j] = cb;
        x[inst * n + j] = dga_argmin_x(cb, lb[inst * lb_stride + j], ub[inst * ub_stride + j]);
    }
}

// out = K v (rows of `ptr`) per instance, one lane per (row, instance), storage order; only_active: instances whose block
// predicate is off are skipped
__global__ __launch_bounds__(kBlock) void k_dgab_product(i64 rows, i64 cols, const i64 *__restrict__ ptr, const i32 *__restrict__ idx,
                                                         const double *__restrict__ val, const double *__restrict__ v,
                                                         const DgaCtl *__restrict__ ctl, int only_active, double *__restrict__ out) {
    const i64 inst = blockIdx.y;
    if (only_active ? !ctl[inst].active : ctl[inst].frozen) return;
    const double *__restrict__ vk = v + inst * cols;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (i64)gridDim.x * blockDim.x)
        out[inst * rows + i] = row_dot<1>(ptr, idx, val, vk, i, 0);
}

// like k_dgab_product over every instance (the report's K x of a frozen instance too)
__global__ __launch_bounds__(kBlock) void k_dgab_product_all(i64 rows, i64 cols, const i64 *__restrict__ ptr, const i32 *__restrict__ idx,
                                                             const double *__restrict__ val, const double *__restrict__ v,
                                                             double *__restrict__ out) {
    const i64 inst = blockIdx.y;
    const double *__restrict__ vk = v + inst * cols;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (i64)gridDim.x * blockDim.x)
        out[inst * rows + i] = row_dot<1>(ptr, idx, val, vk, i, 0);
}

// BB: b holds one vector per instance (slp_batch_dga_set_rhs), b_stride apart; a template parameter, so that a state with a
// shared b launches the code it launched before the switch existed
template <bool BB>
__global__ void k_dgab_grad(i64 m, i64 r0, i64 r1, int ineq, const double *__restrict__ ax, const double *__restrict__ b, i64 b_stride,
                            const double *__restrict__ y, double *__restrict__ g, const DgaCtl *__restrict__ ctl,
                            double *__restrict__ part_gb, double *__restrict__ part_min, int *__restrict__ part_any) {
    __shared__ double red[kBlock / kWave];
    const i64 inst = blockIdx.y;
    if (ctl[inst].frozen) return;
    dga_grad_body(m, r0, r1, ineq, ax + inst * m, BB ? b + inst * b_stride : b, y + inst * m, g + inst * m, part_gb + inst * kDgaParts, part_min + inst * kDgaParts,
                  part_any + inst * kDgaParts, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x,
                  dga_part_tiles(m, (int)blockIdx.x, (int)gridDim.x), red);
}

// one workgroup per instance: the block's scalars; a frozen instance's predicate is off
__global__ void k_dgab_begin(const double *__restrict__ part_gb, const double *__restrict__ part_min, const int *__restrict__ part_any,
                             DgaCtl *__restrict__ ctl) {
    __shared__ double red[kBlock / kWave];
    const i64 inst = blockIdx.x;
    if (ctl[inst].frozen) {
        if (threadIdx.x == 0) { ctl[inst].active = 0; ctl[inst].t = 0.0; }
        return;
    }
    dga_begin_body(kDgaParts, part_gb + inst * kDgaParts, part_min + inst * kDgaParts, part_any + inst * kDgaParts, ctl + inst, (int)threadIdx.x, red);
}

__global__ void k_dgab_update(i64 m, i64 r0, i64 r1, int ineq, const DgaCtl *__restrict__ ctl, const double *__restrict__ g,
                              double *__restrict__ y) {
    const i64 inst = blockIdx.y;
    if (!ctl[inst].active) return;
    const double t = ctl[inst].t;
    for (i64 i = r0 + (i64)blockIdx.x * blockDim.x + threadIdx.x; i < r1; i += (i64)gridDim.x * blockDim.x)
        y[inst * m + i] = dga_update_y(y[inst * m + i], t, g[inst * m + i], ineq);
}

// a workgroup's nan-max of one value per lane, valid in thread 0.  red: kBlock / kWave doubles.  Two barriers.
__device__ __forceinline__ double dgab_block_nanmax(double v, double *red) {
    v = many_wave_nanmax(v);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        r = red[0];
        for (int w = 1; w < kBlock / kWave; ++w) r = nan_max(r, red[w]);
    }
    __syncthreads();
    return r;
}

// k_dgab_update of a check iteration: the same update, and the workgroup's max |y_new - y_old| into its slot `off + blockIdx.x` of
// the instance's `parts` slots; 0.0 from an instance whose block predicate is off.  Frozen and stopped instances write nothing:
// k_dgab_decide does not look at their slots.
__global__ __launch_bounds__(kBlock) void k_dgab_update_step(i64 m, i64 r0, i64 r1, int ineq, const DgaCtl *__restrict__ ctl,
                                                             const double *__restrict__ g, double *__restrict__ y,
                                                             double *__restrict__ step_part, int parts, int off) {
    __shared__ double red[kBlock / kWave];
    const i64 inst = blockIdx.y;
    if (ctl[inst].frozen) return;
    double dy = 0.0;
    if (ctl[inst].active) {
        const double t = ctl[inst].t;
        for (i64 i = r0 + (i64)blockIdx.x * blockDim.x + threadIdx.x; i < r1; i += (i64)gridDim.x * blockDim.x) {
            const double yo = y[inst * m + i], yn = dga_update_y(yo, t, g[inst * m + i], ineq);
            y[inst * m + i] = yn;
            dy = nan_max(dy, fabs(yn - yo));
        }
    }
    dy = dgab_block_nanmax(dy, red);
    if (threadIdx.x == 0) step_part[inst * parts + off + blockIdx.x] = dy;
}

// ---- the stopping test: the bound of the live instances, then the decision --------------------------------------------------------

// k_dgab_energy_x / the y . b of k_dgab_energy_y over the instances that still move
__global__ __launch_bounds__(kBlock) void k_dgab_bound_x(i64 n, const double *__restrict__ cbar, const double *__restrict__ lb, i64 lb_stride,
                                                         const double *__restrict__ ub, i64 ub_stride, const DgaCtl *__restrict__ ctl,
                                                         double *__restrict__ part) {
    __shared__ double red[kBlock / kWave];
    const i64 inst = blockIdx.y;
    if (ctl[inst].frozen) return;
    dga_energy_x_body(n, cbar + inst * n, lb + inst * lb_stride, ub + inst * ub_stride, part + inst * 4 * kDgaParts, red);
}

__global__ __launch_bounds__(kBlock) void k_dgab_bound_y(i64 m, i64 m_eq, const double *__restrict__ y, const double *__restrict__ b,
                                                         i64 b_stride, const DgaCtl *__restrict__ ctl, double *__restrict__ part) {
    __shared__ double red[kBlock / kWave];
    const i64 inst = blockIdx.y;
    if (ctl[inst].frozen) return;
    dga_energy_y_body<false>(m, m_eq, y + inst * m, b + inst * b_stride, nullptr, part + inst * 4 * kDgaParts + kDgaParts, red);
}

// One workgroup per instance, at the end of check iteration `done`: the step from the instance's slots, the bound from the 4
// kDgaParts partial results (targets != NULL: the bound is armed), the record, and the mark that retires the instance.
__global__ __launch_bounds__(kBlock) void k_dgab_decide(DgaCtl *__restrict__ ctl, DgabStop *__restrict__ rec, i64 done, double tol,
                                                        const double *__restrict__ targets, const double *__restrict__ step_part,
                                                        int parts, const double *__restrict__ rpart) {
    __shared__ double red[kBlock / kWave];
    __shared__ double h[4 * kDgaParts];
    const i64 inst = blockIdx.x;
    if (ctl[inst].frozen) return;
    double dy = 0.0;
    for (int i = (int)threadIdx.x; i < parts; i += kBlock) dy = nan_max(dy, step_part[inst * parts + i]);
    const double step = dgab_block_nanmax(dy, red);
    if (targets) {
        for (int i = (int)threadIdx.x; i < 4 * kDgaParts; i += kBlock) h[i] = rpart[inst * 4 * kDgaParts + i];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    int reason = 0;
    const bool sound = !(ctl[inst].flags & DGA_NAN);   // an instance that has met a NaN breakpoint or step certifies nothing
    rec[inst].step = step;
    if (sound && tol >= 0.0 && step <= tol) reason |= 1;   // false for a NaN
    if (targets) {
        const double bound = dga_bound_finish(h), target = targets[inst];
        rec[inst].bound = bound;
        if (sound && target < __builtin_inf() && bound >= target) reason |= 2;   // false for a NaN
    }
    if (reason) {
        rec[inst].done = done;
        rec[inst].reason = reason;
        ctl[inst].frozen = kDgaStopped;
    }
}

// ---- the search, general form: grids of (.., B) over B segments of n ---------------------------------------------------------

// keys of the instance's segment; its end offset for the sort: an instance whose predicate is off has an empty segment
__global__ void k_dgab_keys(int n, const double *__restrict__ d, const double *__restrict__ cbar, unsigned long long *__restrict__ keys,
                            int *__restrict__ cols, DgaCtl *__restrict__ ctl, unsigned int *__restrict__ seg_end) {
    const i64 inst = blockIdx.y;
    const int active = ctl[inst].active;
    if (blockIdx.x == 0 && threadIdx.x == 0) seg_end[inst] = (unsigned int)(inst * n + (active ? n : 0));
    if (!active) return;
    dga_keys_body(n, d + inst * n, cbar + inst * n, keys + inst * n, cols + inst * n, ctl + inst);
}

// global sort: the instance of a global index (the key of the second pass)
struct InstanceOf {
    unsigned int n;
    __device__ unsigned int operator()(unsigned int v) const { return v / n; }
};

__global__ void k_dgab_iota(i64 total, unsigned int *__restrict__ out) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (i64)gridDim.x * blockDim.x) out[i] = (unsigned int)i;
}

// global sort: position i lies in the segment of instance i / n; its global index -> the column inside the instance
__global__ void k_dgab_localise(i64 total, i64 n, int *__restrict__ cols) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (i64)gridDim.x * blockDim.x)
        cols[i] = (int)((i64)(unsigned int)cols[i] - (i / n) * n);
}

__global__ void k_dgab_tile_sums(int n, int tiles, const DgaCtl *__restrict__ ctl, const int *__restrict__ cols, const double *__restrict__ d,
                                 const double *__restrict__ lb, i64 lb_stride, const double *__restrict__ ub, i64 ub_stride,
                                 double *__restrict__ tot_f, double *__restrict__ tot_b) {
    __shared__ double lds[kBlock / kWave];
    const i64 inst = blockIdx.y;
    if (!ctl[inst].active) return;
    dga_tile_sums_body(ctl + inst, cols + inst * n, d + inst * n, lb + inst * lb_stride, ub + inst * ub_stride, tot_f + inst * tiles,
                       tot_b + inst * tiles, lds);
}

__global__ void k_dgab_tile_offsets(int tiles, const DgaCtl *__restrict__ ctl, double *__restrict__ tot_f, double *__restrict__ tot_b) {
    __shared__ double lds[kBlock / kWave];
    const i64 inst = blockIdx.x;
    if (!ctl[inst].active) return;
    const int used = (ctl[inst].nb + kDgaTile - 1) / kDgaTile;
    scan_tile_sums(used, tot_f + inst * tiles, lds);
    scan_tile_sums(used, tot_b + inst * tiles, lds);
}

__global__ void k_dgab_scans(int n, int tiles, const DgaCtl *__restrict__ ctl, const int *__restrict__ cols, const double *__restrict__ d,
                             const double *__restrict__ lb, i64 lb_stride, const double *__restrict__ ub, i64 ub_stride,
                             const double *__restrict__ off_f, const double *__restrict__ off_b, double *__restrict__ F,
                             double *__restrict__ B) {
    __shared__ double lds[kBlock / kWave];
    const i64 inst = blockIdx.y;
    if (!ctl[inst].active) return;
    dga_scans_body(ctl + inst, cols + inst * n, d + inst * n, lb + inst * lb_stride, ub + inst * ub_stride, off_f + inst * tiles,
                   off_b + inst * tiles, F + inst * n, B + inst * n, lds);
}

// one wave per instance, its first lane bisects
__global__ void k_dgab_search(int n, DgaCtl *__restrict__ ctl, const int *__restrict__ cols, const double *__restrict__ cbar,
                              const double *__restrict__ d, const double *__restrict__ F, const double *__restrict__ B,
                              const double *__restrict__ rnd, unsigned long long rnd_base, unsigned long long rnd_count, int ineq) {
    const i64 inst = blockIdx.x;
    if (!ctl[inst].active || threadIdx.x != 0) return;
    dga_search_body(ctl + inst, cols + inst * n, cbar + inst * n, d + inst * n, F + inst * n, B + inst * n, rnd, rnd_base, rnd_count, ineq);
}

// ---- the search, fused form: one workgroup per instance -------------------------------------------------------------------------

__global__ void __launch_bounds__(kDgaFusedThreads)
k_dgab_fused(int n, int npad, const double *__restrict__ d, const double *__restrict__ cbar, const double *__restrict__ lb, i64 lb_stride,
             const double *__restrict__ ub, i64 ub_stride, DgaCtl *__restrict__ ctl, const double *__restrict__ rnd,
             unsigned long long rnd_base, unsigned long long rnd_count, int ineq) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dga_lds[];
    const i64 inst = blockIdx.x;
    if (!ctl[inst].active) return;
    dga_fused_body(n, npad, d + inst * n, cbar + inst * n, lb + inst * lb_stride, ub + inst * ub_stride, ctl + inst, rnd, rnd_base, rnd_count,
                   ineq, dga_lds);
}

// ---- report: 4 kDgaParts partial results per instance ---------------------------------------------------------------------------

__global__ void k_dgab_energy_x(i64 n, const double *__restrict__ cbar, const double *__restrict__ lb, i64 lb_stride,
                                const double *__restrict__ ub, i64 ub_stride, double *__restrict__ part) {
    __shared__ double red[kBlock / kWave];
    const i64 inst = blockIdx.y;
    dga_energy_x_body(n, cbar + inst * n, lb + inst * lb_stride, ub + inst * ub_stride, part + inst * 4 * kDgaParts, red);
}

__global__ void k_dgab_energy_y(i64 m, i64 m_eq, const double *__restrict__ y, const double *__restrict__ b, i64 b_stride, const double *__restrict__ ax,
                                double *__restrict__ part) {
    __shared__ double red[kBlock / kWave];
    const i64 inst = blockIdx.y;
    dga_energy_y_body(m, m_eq, y + inst * m, b + inst * b_stride, ax + inst * m, part + inst * 4 * kDgaParts + kDgaParts, red);
}

}  // namespace

struct slp_batch_dga {
    slp_matrix *k = nullptr;   // borrowed
    i64 n = 0, m = 0, m_eq = 0, B = 0;
    i64 lb_stride = 0, ub_stride = 0;   // n when the bounds are per instance, 0 when all instances share them
    i64 b_stride = 0;                   // m when the right-hand sides are per instance (slp_batch_dga_set_rhs), 0 when shared
    DevBuf<double> b, c, lb, ub, y, x, cbar, ax, g, d, rcbar, rx, rax, rpart;
    DevBuf<DgaCtl> ctl;
    DevBuf<double> part_gb, part_min;
    DevBuf<int> part_any;
    // the search
    bool fused = false;
    int npad = 0, tiles = 0;
    DevBuf<double> F, Bw, tot_f, tot_b;
    DevBuf<int> cols, cols_sorted;
    DevBuf<unsigned long long> keys, keys_sorted;
    DevBuf<unsigned int> seg_begin, seg_end;
    DevBuf<unsigned char> sort_tmp;
    size_t sort_bytes = 0;
    bool sort_global = false;              // two device-wide stable sorts instead of the segmented one
    int inst_bits = 1;                     // bits of an instance index
    DevBuf<unsigned int> gidx, gidx_sorted;   // global sort: i = instance * n + column, and its order by key
    size_t sort_bytes1 = 0, sort_bytes2 = 0;
    // the shared stream of tie draws
    DevBuf<double> rnd;
    DgaDrawWindow draws;   // the host's view of rnd (slp_dga_draws.h)
    i64 iters = 0;
    // the stopping test: off while !armed.  Its buffers are allocated at the first arming.
    bool armed = false, ever_armed = false, has_targets = false;
    double tol = -1.0;      // < 0: the step does not stop
    i64 check_every = 1;
    int step_parts_ineq = 0, step_parts_eq = 0;   // workgroups (= step slots) of the update pass per block of rows
    DevBuf<DgabStop> stop;
    DevBuf<double> targets, step_part;
    StageTimer timer;
};

namespace {

// Automatic rules, from profiles/dga_batch.json (Potts-50: n = 7400, Potts-256: n = 196 096; B = 1, 8, 32, 64, 256).
// Sort of the general search: the global one wherever the general search is the automatic choice (n > kDgaFusedAuto); it is
// 1.35 x (B = 256) to 57 x (B = 1) the segmented one's speed at n = 196 096 and 3.5 x (B = 1) to 1.0 x (B = 256) at n = 7400;
// unmeasured between 2048 and 7400.  SLP_DGA_BATCH_SORT=segmented|global overrides.
constexpr i64 kDgabGlobalSortFrom = kDgaFusedAuto;
// Path: fused up to kDgaFusedAuto variables as the single solver, and up to kDgaFusedMax from kDgabFusedBatch instances on: at
// n = 7400 one workgroup per instance is 0.63 x / 0.84 x the general search at B = 1 / 8 and 1.43 x / 1.75 x / 1.94 x at
// B = 32 / 64 / 256 (the cross-over lies between 8 and 32 instances).
constexpr i64 kDgabFusedBatch = 32;

dim3 grid2(i64 work, i64 batch) { return dim3((unsigned)grid_for(work, kBlock), (unsigned)batch); }

bool auto_fused(i64 n, i64 batch) { return n <= kDgaFusedAuto || (n <= kDgaFusedMax && batch >= kDgabFusedBatch); }

void dgab_search_setup(slp_batch_dga *s, int path) {
    const i64 n = s->n, B = s->B;
    SLP_REQUIRE(path >= 0 && path <= 2, "batched dual gradient ascent: path must be 0 (auto), 1 (fused) or 2 (general)");
    SLP_REQUIRE(path != 1 || n <= kDgaFusedMax, "batched dual gradient ascent: the fused search holds at most 8192 variables");
    const bool fused = path == 1 || (path == 0 && auto_fused(n, B));
    if (fused) {
        SLP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dgab_fused), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)fused_lds_bytes(kDgaFusedMax)));
        s->fused = true;
        return;
    }
    SLP_REQUIRE((double)n * (double)B < 2147483647.0, "batched dual gradient ascent: the general search sorts at most 2^31 - 1 keys per launch");
    // the sort of the general search: "segmented" (one workgroup sorts a segment) or "global" (all keys in one device-wide
    // stable sort, then a stable sort by instance); the automatic choice is by the segment length
    int sort = 0;
    if (const char *e = getenv("SLP_DGA_BATCH_SORT")) sort = !strcmp(e, "segmented") ? 1 : (!strcmp(e, "global") ? 2 : 0);
    s->sort_global = sort == 2 || (sort == 0 && n > kDgabGlobalSortFrom);
    const size_t nb = (size_t)n * (size_t)B, tb = (size_t)s->tiles * (size_t)B;
    if (!s->keys.p) {
        s->F.alloc(nb); s->Bw.alloc(nb); s->tot_f.alloc(tb); s->tot_b.alloc(tb);
        s->cols.alloc(nb); s->cols_sorted.alloc(nb); s->keys.alloc(nb); s->keys_sorted.alloc(nb);
        std::vector<unsigned int> begin((size_t)B);
        for (i64 k = 0; k < B; ++k) begin[(size_t)k] = (unsigned int)(k * n);
        s->seg_begin.upload(begin.data(), (size_t)B);
        s->seg_end.alloc((size_t)B);
    }
    size_t need = 0;
    if (s->sort_global) {
        if (!s->gidx.p) {
            s->gidx.alloc(nb); s->gidx_sorted.alloc(nb);
            hipLaunchKernelGGL(k_dgab_iota, dim3(grid_for((i64)nb, kBlock)), dim3(kBlock), 0, ctx().stream, (i64)nb, s->gidx.p);
            SLP_HIP(hipGetLastError());
            s->inst_bits = 1;
            while (((i64)1 << s->inst_bits) < B) ++s->inst_bits;
        }
        SLP_HIP(rocprim::radix_sort_pairs(nullptr, s->sort_bytes1, s->keys.p, s->keys_sorted.p, s->gidx.p, s->gidx_sorted.p, nb, 0u, 64u,
                                          ctx().stream));
        SLP_HIP(rocprim::radix_sort_pairs(nullptr, s->sort_bytes2, rocprim::make_transform_iterator(s->gidx_sorted.p, InstanceOf{(unsigned int)n}),
                                          reinterpret_cast<unsigned int *>(s->cols.p), s->gidx_sorted.p,
                                          reinterpret_cast<unsigned int *>(s->cols_sorted.p), nb, 0u, (unsigned int)s->inst_bits, ctx().stream));
        need = std::max(s->sort_bytes1, s->sort_bytes2);
    } else {
        SLP_HIP(rocprim::segmented_radix_sort_pairs(nullptr, s->sort_bytes, s->keys.p, s->keys_sorted.p, s->cols.p, s->cols_sorted.p,
                                                    (unsigned int)nb, (unsigned int)B, s->seg_begin.p, s->seg_end.p, 0u, 64u, ctx().stream));
        need = s->sort_bytes;
    }
    if (s->sort_tmp.n < need || !s->sort_tmp.p) s->sort_tmp.alloc(need ? need : 1);
    s->fused = false;
}

// c_bar and x of the multipliers into (cbar, x)
void dgab_argmin(slp_batch_dga *s, double *cbar, double *x, int skip_frozen) {
    const CsrDev &at = s->k->at;
    hipLaunchKernelGGL(k_dgab_cols, grid2(s->n, s->B), dim3(kBlock), 0, ctx().stream, s->n, s->m, s->m_eq, at.ptr.p, at.idx.p, at.val.p, s->y.p,
                       s->c.p, s->lb.p, s->lb_stride, s->ub.p, s->ub_stride, s->ctl.p, skip_frozen, cbar, x);
    SLP_HIP(hipGetLastError());
}

// `check`: the update pass of a check iteration, which also leaves the step in the block's slots
void dgab_block(slp_batch_dga *s, i64 r0, i64 r1, int ineq, bool check) {
    hipStream_t st = ctx().stream;
    const CsrDev &at = s->k->at;
    const i64 n = s->n, m = s->m, B = s->B;
    const unsigned int ub = (unsigned int)B;
    hipLaunchKernelGGL(s->b_stride ? k_dgab_grad<true> : k_dgab_grad<false>, dim3(kDgaParts, ub), dim3(kBlock), 0, st, m, r0, r1, ineq, s->ax.p,
                       s->b.p, s->b_stride, s->y.p, s->g.p, s->ctl.p, s->part_gb.p, s->part_min.p, s->part_any.p);
    hipLaunchKernelGGL(k_dgab_begin, dim3(ub), dim3(kBlock), 0, st, s->part_gb.p, s->part_min.p, s->part_any.p, s->ctl.p);
    s->timer.mark(ST_REST);
    hipLaunchKernelGGL(k_dgab_product, grid2(n, B), dim3(kBlock), 0, st, n, m, at.ptr.p, at.idx.p, at.val.p, s->g.p, s->ctl.p, 1, s->d.p);
    SLP_HIP(hipGetLastError());
    s->timer.mark(ST_PRODUCTS);
    const unsigned long long rb = s->draws.base, rc = s->draws.size();
    if (s->fused) {
        hipLaunchKernelGGL(k_dgab_fused, dim3(ub), dim3(kDgaFusedThreads), fused_lds_bytes(s->npad), st, (int)n, s->npad, s->d.p, s->cbar.p,
                           s->lb.p, s->lb_stride, s->ub.p, s->ub_stride, s->ctl.p, s->rnd.p, rb, rc, ineq);
        SLP_HIP(hipGetLastError());
        s->timer.mark(ST_FUSED);
    } else {
        const unsigned int tiles = (unsigned int)s->tiles;
        hipLaunchKernelGGL(k_dgab_keys, grid2(n, B), dim3(kBlock), 0, st, (int)n, s->d.p, s->cbar.p, s->keys.p, s->cols.p, s->ctl.p,
                           s->seg_end.p);
        SLP_HIP(hipGetLastError());
        s->timer.mark(ST_REST);
        if (s->sort_global) {
            // stable by key over all instances, then stable by instance: segment k holds instance k's columns in key order, equal
            // keys in column order -- the order of the segmented sort and of the single solver's
            const size_t total = (size_t)n * (size_t)B;
            size_t bytes = s->sort_bytes1;
            SLP_HIP(rocprim::radix_sort_pairs(s->sort_tmp.p, bytes, s->keys.p, s->keys_sorted.p, s->gidx.p, s->gidx_sorted.p, total, 0u, 64u, st));
            bytes = s->sort_bytes2;
            SLP_HIP(rocprim::radix_sort_pairs(s->sort_tmp.p, bytes, rocprim::make_transform_iterator(s->gidx_sorted.p, InstanceOf{(unsigned int)n}),
                                              reinterpret_cast<unsigned int *>(s->cols.p), s->gidx_sorted.p,
                                              reinterpret_cast<unsigned int *>(s->cols_sorted.p), total, 0u, (unsigned int)s->inst_bits, st));
            hipLaunchKernelGGL(k_dgab_localise, dim3(grid_for((i64)total, kBlock)), dim3(kBlock), 0, st, (i64)total, n, s->cols_sorted.p);
            SLP_HIP(hipGetLastError());
        } else {
            size_t bytes = s->sort_bytes;
            SLP_HIP(rocprim::segmented_radix_sort_pairs(s->sort_tmp.p, bytes, s->keys.p, s->keys_sorted.p, s->cols.p, s->cols_sorted.p,
                                                        (unsigned int)(n * B), ub, s->seg_begin.p, s->seg_end.p, 0u, 64u, st));
        }
        s->timer.mark(ST_SORT);
        hipLaunchKernelGGL(k_dgab_tile_sums, dim3(tiles, ub), dim3(kBlock), 0, st, (int)n, s->tiles, s->ctl.p, s->cols_sorted.p, s->d.p, s->lb.p,
                           s->lb_stride, s->ub.p, s->ub_stride, s->tot_f.p, s->tot_b.p);
        hipLaunchKernelGGL(k_dgab_tile_offsets, dim3(ub), dim3(kBlock), 0, st, s->tiles, s->ctl.p, s->tot_f.p, s->tot_b.p);
        hipLaunchKernelGGL(k_dgab_scans, dim3(tiles, ub), dim3(kBlock), 0, st, (int)n, s->tiles, s->ctl.p, s->cols_sorted.p, s->d.p, s->lb.p,
                           s->lb_stride, s->ub.p, s->ub_stride, s->tot_f.p, s->tot_b.p, s->F.p, s->Bw.p);
        SLP_HIP(hipGetLastError());
        s->timer.mark(ST_SCANS);
        hipLaunchKernelGGL(k_dgab_search, dim3(ub), dim3(kWave), 0, st, (int)n, s->ctl.p, s->cols_sorted.p, s->cbar.p, s->d.p, s->F.p, s->Bw.p,
                           s->rnd.p, rb, rc, ineq);
        SLP_HIP(hipGetLastError());
        s->timer.mark(ST_REST);
    }
    if (check)
        hipLaunchKernelGGL(k_dgab_update_step, grid2(r1 - r0, B), dim3(kBlock), 0, st, m, r0, r1, ineq, s->ctl.p, s->g.p, s->y.p, s->step_part.p,
                           s->step_parts_ineq + s->step_parts_eq, ineq ? 0 : s->step_parts_ineq);
    else
        hipLaunchKernelGGL(k_dgab_update, grid2(r1 - r0, B), dim3(kBlock), 0, st, m, r0, r1, ineq, s->ctl.p, s->g.p, s->y.p);
    SLP_HIP(hipGetLastError());
    s->timer.mark(ST_REST);
}

// behind the updates of check iteration `done`: the bound of the live instances when cut-offs were given, then the decision
void dgab_check(slp_batch_dga *s, i64 done) {
    hipStream_t st = ctx().stream;
    const unsigned int ub = (unsigned int)s->B;
    if (s->has_targets) {
        dgab_argmin(s, s->rcbar.p, s->rx.p, 1);
        s->timer.mark(ST_PRODUCTS);
        hipLaunchKernelGGL(k_dgab_bound_x, dim3(kDgaParts, ub), dim3(kBlock), 0, st, s->n, s->rcbar.p, s->lb.p, s->lb_stride, s->ub.p, s->ub_stride,
                           s->ctl.p, s->rpart.p);
        hipLaunchKernelGGL(k_dgab_bound_y, dim3(kDgaParts, ub), dim3(kBlock), 0, st, s->m, s->m_eq, s->y.p, s->b.p, s->b_stride, s->ctl.p, s->rpart.p);
    }
    hipLaunchKernelGGL(k_dgab_decide, dim3(ub), dim3(kBlock), 0, st, s->ctl.p, s->stop.p, done, s->tol, s->has_targets ? s->targets.p : nullptr,
                       s->step_part.p, s->step_parts_ineq + s->step_parts_eq, s->rpart.p);
    SLP_HIP(hipGetLastError());
    s->timer.mark(ST_REST);
}

void dgab_iteration(slp_batch_dga *s, bool check = false) {
    const CsrDev &a = s->k->a;
    s->timer.mark(-1);
    dgab_argmin(s, s->cbar.p, s->x.p, 1);
    hipLaunchKernelGGL(k_dgab_product, grid2(s->m, s->B), dim3(kBlock), 0, ctx().stream, s->m, s->n, a.ptr.p, a.idx.p, a.val.p, s->x.p, s->ctl.p,
                       0, s->ax.p);
    SLP_HIP(hipGetLastError());
    s->timer.mark(ST_PRODUCTS);
    if (s->m > s->m_eq) dgab_block(s, s->m_eq, s->m, 1, check);
    if (s->m_eq > 0) dgab_block(s, 0, s->m_eq, 0, check);
    if (check) dgab_check(s, s->iters + 1);
}

// the controls of all instances; refreshes the bound on the draws taken
void dgab_read_ctl(slp_batch_dga *s, std::vector<DgaCtl> &h) {
    h.resize((size_t)s->B);
    s->ctl.download(h.data(), (size_t)s->B);
    // a frozen instance and a stopped one stand still: no readers of the stream (slp_dga_draws.h)
    s->draws.observe(dga_furthest_reader(h.size(), [&](size_t k) { return !h[k].frozen; }, [&](size_t k) { return (uint64_t)h[k].consumed; }));
}

void dgab_report(slp_batch_dga *s, double *out) {
    hipStream_t st = ctx().stream;
    const CsrDev &a = s->k->a;
    const size_t nb = (size_t)s->n * (size_t)s->B, mb = (size_t)s->m * (size_t)s->B;
    if (!s->rcbar.p) { s->rcbar.alloc(nb); s->rx.alloc(nb); s->rax.alloc(mb); s->rpart.alloc((size_t)4 * kDgaParts * (size_t)s->B); }
    const unsigned int ub = (unsigned int)s->B;
    dgab_argmin(s, s->rcbar.p, s->rx.p, 0);
    hipLaunchKernelGGL(k_dgab_product_all, grid2(s->m, s->B), dim3(kBlock), 0, st, s->m, s->n, a.ptr.p, a.idx.p, a.val.p, s->rx.p, s->rax.p);
    hipLaunchKernelGGL(k_dgab_energy_x, dim3(kDgaParts, ub), dim3(kBlock), 0, st, s->n, s->rcbar.p, s->lb.p, s->lb_stride, s->ub.p, s->ub_stride,
                       s->rpart.p);
    hipLaunchKernelGGL(k_dgab_energy_y, dim3(kDgaParts, ub), dim3(kBlock), 0, st, s->m, s->m_eq, s->y.p, s->b.p, s->b_stride, s->rax.p, s->rpart.p);
    SLP_HIP(hipGetLastError());
    std::vector<double> h((size_t)4 * kDgaParts * (size_t)s->B);
    s->rpart.download(h.data(), h.size());
    for (i64 k = 0; k < s->B; ++k) dga_report_finish(h.data() + (size_t)k * 4 * kDgaParts, true, out + 3 * k);
}

}  // namespace

extern "C" {

slp_batch_dga *slp_batch_dga_create_on(slp_matrix *a, int64_t m_eq, const double *b, int64_t batch, const double *c, const double *lb,
                                       int lb_batched, const double *ub, int ub_batched, const double *y0, int y0_batched) {
    SLP_API_PTR({
        SLP_REQUIRE(a && b && c && lb && ub && y0, "slp_batch_dga_create_on: NULL argument");
        SLP_REQUIRE(batch >= 1, "slp_batch_dga_create_on: batch must be at least 1");
        SLP_REQUIRE(batch <= 65535, "slp_batch_dga_create_on: at most 65535 instances");
        const i64 m = a->a.nrow, n = a->a.ncol, nnz = a->a.nnz;
        SLP_REQUIRE(m >= 1, "slp_batch_dga_create_on: the LP has no constraint rows");
        SLP_REQUIRE(m_eq >= 0 && m_eq <= m, "slp_batch_dga_create_on: m_eq out of range");
        SLP_REQUIRE(a->chunks.empty() && !a->csr_released,
                    "slp_batch_dga_create_on: the batch walks the CSR arrays; a chunked matrix or one whose CSR was released has none");
        SLP_REQUIRE(n > 0 && n < ((i64)1 << 31) - kDgaTile, "slp_batch_dga_create_on: the number of variables must be in 1 .. 2^31 - 1025");
        int path = 0;
        if (const char *e = getenv("SLP_DGA_BATCH_PATH")) path = !strcmp(e, "fused") ? 1 : (!strcmp(e, "general") ? 2 : 0);
        SLP_REQUIRE(path != 1 || n <= kDgaFusedMax, "slp_batch_dga_create_on: the fused search holds at most 8192 variables");
        // nothing is allocated before this check: per (instance, variable) c, x, c_bar, d and the report's two (8 B each), lb and ub
        // when per instance, the general search's keys, columns and scans (40 B) and about as much again for the sort; per
        // (instance, row) y, K x, g and the report's K x; the transposed CSR; the partial results
        {
            i64 free_b = 0, total_b = 0;
            SLP_REQUIRE(slp_device_memory(&free_b, &total_b) == 0, slp_last_error());
            const double per_var = 48.0 + 8.0 * ((lb_batched ? 1 : 0) + (ub_batched ? 1 : 0)) + 80.0;
            const double need = ((double)n * per_var + (double)m * 32.0 + 8.0 * 7.0 * kDgaParts + sizeof(DgaCtl)) * (double)batch +
                                20.0 * (double)nnz + 8.0 * (double)(n + m + 2) + 8.0 * (double)(2 * n + m);
            const double have = (double)free_b + (double)slp_cached_bytes();
            if (need > have)
                throw Error("slp_batch_dga_create_on: " + std::to_string(batch) + " instances need " + std::to_string(need / 1e9) +
                            " GB of device memory, " + std::to_string(have / 1e9) + " GB are free");
        }
        auto *s = new slp_batch_dga();
        try {
            s->k = a; s->n = n; s->m = m; s->m_eq = m_eq; s->B = batch;
            s->lb_stride = lb_batched ? n : 0;
            s->ub_stride = ub_batched ? n : 0;
            int npad = 64;
            while (npad < n && npad < (1 << 30)) npad <<= 1;
            s->npad = npad;
            s->tiles = (int)((n + kDgaTile - 1) / kDgaTile);
            build_transpose(a);
            const size_t sn = (size_t)n, sm = (size_t)m, sb = (size_t)batch;
            s->ctl.alloc(sb);
            s->ctl.zero();
            dgab_search_setup(s, path);
            s->c.upload(c, sn * sb);
            s->lb.upload(lb, lb_batched ? sn * sb : sn);
            s->ub.upload(ub, ub_batched ? sn * sb : sn);
            s->b.upload(b, sm);
            if (y0_batched) {
                s->y.upload(y0, sm * sb);
            } else {
                std::vector<double> rep(sm * sb);
                for (size_t k = 0; k < sb; ++k) std::copy(y0, y0 + sm, rep.begin() + (ptrdiff_t)(k * sm));
                s->y.upload(rep.data(), rep.size());
            }
            s->x.alloc(sn * sb); s->cbar.alloc(sn * sb); s->d.alloc(sn * sb);
            s->ax.alloc(sm * sb); s->g.alloc(sm * sb);
            s->part_gb.alloc((size_t)kDgaParts * sb); s->part_min.alloc((size_t)kDgaParts * sb); s->part_any.alloc((size_t)kDgaParts * sb);
            dgab_argmin(s, s->cbar.p, s->x.p, 0);   // the x of y0: what a frozen instance keeps
            // a start whose dual energy is -inf freezes its instance (the single solve returns at once, :133-139)
            std::vector<double> rep(3 * sb);
            dgab_report(s, rep.data());
            std::vector<DgaCtl> h(sb);
            memset(h.data(), 0, sb * sizeof(DgaCtl));
            for (size_t k = 0; k < sb; ++k) h[k].frozen = rep[3 * k] == -INFINITY;
            s->ctl.upload(h.data(), sb);
        } catch (...) {
            delete s;
            throw;
        }
        ++a->borrowers;
        ++a->csr_bound;
        return s;
    })
}

void slp_batch_dga_destroy(slp_batch_dga *s) {
    if (!s) return;
    --s->k->borrowers;
    --s->k->csr_bound;
    delete s;
}

int slp_batch_dga_set_path(slp_batch_dga *s, int path) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_batch_dga_set_path: NULL handle");
        dgab_search_setup(s, path);
        SLP_HIP(hipStreamSynchronize(ctx().stream));
    })
}

int slp_batch_dga_path(const slp_batch_dga *s) { return s ? (s->fused ? 1 : 2) : -1; }

int slp_batch_dga_sort(const slp_batch_dga *s) { return s ? (s->fused ? 0 : (s->sort_global ? 2 : 1)) : -1; }

int slp_batch_dga_iterate(slp_batch_dga *s, int64_t k) {
    SLP_API_INT({
        SLP_REQUIRE(s && k >= 0, "slp_batch_dga_iterate: bad arguments");
        if (s->ever_armed) {   // when every instance is stopped or frozen nothing is launched and the count of iterations stays
            std::vector<DgaCtl> h;
            dgab_read_ctl(s, h);
            if (std::all_of(h.begin(), h.end(), [](const DgaCtl &c) { return c.frozen != 0; })) return 0;
        }
        for (i64 it = 0; it < k && s->draws.reserve(1); ++it) {   // at most two tie draws per instance and iteration
            dgab_iteration(s, s->armed && (s->iters + 1) % s->check_every == 0);
            ++s->iters;
        }
    })
}

int64_t slp_batch_dga_iterations(const slp_batch_dga *s) { return s ? s->iters : -1; }

int slp_batch_dga_push_random(slp_batch_dga *s, const double *draws, int64_t count) {
    SLP_API_INT({
        SLP_REQUIRE(s && count >= 0 && (draws || count == 0), "slp_batch_dga_push_random: bad arguments");
        std::vector<DgaCtl> h;
        dgab_read_ctl(s, h);
        dga_push_draws(h, [](size_t) { return 0ull; }, s->draws, s->rnd, draws, count, kDropFirst);
    })
}

int slp_batch_dga_status(slp_batch_dga *s, int64_t *out) {
    SLP_API_INT({
        SLP_REQUIRE(s && out, "slp_batch_dga_status: NULL argument");
        std::vector<DgaCtl> h;
        dgab_read_ctl(s, h);
        dga_status_out(h, s->draws, s->iters, out);
    })
}

int slp_batch_dga_frozen(slp_batch_dga *s, int32_t *out) {
    SLP_API_INT({
        SLP_REQUIRE(s && out, "slp_batch_dga_frozen: NULL argument");
        std::vector<DgaCtl> h;
        dgab_read_ctl(s, h);
        for (size_t k = 0; k < h.size(); ++k) out[k] = h[k].frozen == 1;   // (kDgaStopped: retired by the stopping test, not frozen)
    })
}

int slp_batch_dga_get_x(slp_batch_dga *s, double *x) {
    SLP_API_INT({ SLP_REQUIRE(s && x, "NULL argument"); s->x.download(x, (size_t)s->n * (size_t)s->B); })
}

int slp_batch_dga_get_y(slp_batch_dga *s, double *y) {
    SLP_API_INT({ SLP_REQUIRE(s && y, "NULL argument"); s->y.download(y, (size_t)s->m * (size_t)s->B); })
}

int slp_batch_dga_report(slp_batch_dga *s, double *out) {
    SLP_API_INT({
        SLP_REQUIRE(s && out, "slp_batch_dga_report: NULL argument");
        dgab_report(s, out);
    })
}

int slp_batch_dga_set_rhs(slp_batch_dga *s, const double *b, int b_batched) {
    SLP_API_INT({
        SLP_REQUIRE(s && b, "slp_batch_dga_set_rhs: NULL argument");
        SLP_REQUIRE(s->iters == 0, "slp_batch_dga_set_rhs: the state has iterated; the right-hand sides are set before the first iteration");
        const size_t sm = (size_t)s->m, sb = (size_t)s->B, count = b_batched ? sm * sb : sm;
        SLP_HIP(hipStreamSynchronize(ctx().stream));
        DevBuf<double> nb;
        if (count > s->b.n) {   // nothing is allocated before this check; a refusal leaves the old right-hand sides in place
            i64 free_b = 0, total_b = 0;
            SLP_REQUIRE(slp_device_memory(&free_b, &total_b) == 0, slp_last_error());
            const double need = 8.0 * (double)count, have = (double)free_b + (double)slp_cached_bytes();
            if (need > have)
                throw Error("slp_batch_dga_set_rhs: per-instance right-hand sides need " + std::to_string(need / 1e9) +
                            " GB of device memory, " + std::to_string(have / 1e9) + " GB are free");
            nb.alloc(count);
            nb.upload(b, count);
            s->b = std::move(nb);
        } else {
            s->b.upload(b, count);
        }
        s->b_stride = b_batched ? s->m : 0;
        // what the constructor derived from b: a start whose dual energy is -inf freezes its instance
        std::vector<double> rep(3 * sb);
        dgab_report(s, rep.data());
        std::vector<DgaCtl> h(sb);
        s->ctl.download(h.data(), sb);
        for (size_t k = 0; k < sb; ++k) h[k].frozen = rep[3 * k] == -INFINITY;
        s->ctl.upload(h.data(), sb);
    })
}

int slp_batch_dga_set_stop(slp_batch_dga *s, double tol, const double *targets, int64_t check_every) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_batch_dga_set_stop: NULL handle");
        SLP_REQUIRE(std::isfinite(tol), "slp_batch_dga_set_stop: tol must be finite (tol < 0 turns the step test off)");
        const bool arm = tol >= 0.0 || targets;
        SLP_REQUIRE(!arm || check_every >= 1, "slp_batch_dga_set_stop: check_every must be at least 1");
        const size_t sb = (size_t)s->B;
        for (size_t k = 0; targets && k < sb; ++k)
            SLP_REQUIRE(targets[k] == targets[k] && targets[k] != -INFINITY,
                        "slp_batch_dga_set_stop: a cut-off is NaN or -inf (+inf: the instance has none)");
        SLP_HIP(hipStreamSynchronize(ctx().stream));
        if (arm && !s->stop.p) {   // the records and the step slots, at the first arming
            const std::vector<DgabStop> rec(sb, DgabStop{0, __builtin_inf(), -__builtin_inf(), 0, 0});
            s->stop.upload(rec.data(), sb);
            s->step_parts_ineq = s->m > s->m_eq ? grid_for(s->m - s->m_eq, kBlock) : 0;
            s->step_parts_eq = s->m_eq > 0 ? grid_for(s->m_eq, kBlock) : 0;
            s->step_part.alloc((size_t)(s->step_parts_ineq + s->step_parts_eq) * sb);
            s->ever_armed = true;
        }
        if (targets) s->targets.upload(targets, sb);
        // the marks stay: a stopped instance cannot be resumed
        s->armed = arm;
        s->has_targets = targets != nullptr;
        s->tol = tol < 0.0 ? -1.0 : tol;
        if (arm) s->check_every = check_every;
    })
}

int slp_batch_dga_stop_state(slp_batch_dga *s, int64_t *iterations, int32_t *reason, double *step, double *bound) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_batch_dga_stop_state: NULL handle");
        std::vector<DgaCtl> h;
        dgab_read_ctl(s, h);   // synchronises
        std::vector<DgabStop> rec((size_t)s->B, DgabStop{0, __builtin_inf(), -__builtin_inf(), 0, 0});
        if (s->stop.p) s->stop.download(rec.data(), rec.size());
        for (size_t k = 0; k < rec.size(); ++k) {
            const bool stopped = h[k].frozen == kDgaStopped;
            if (iterations) iterations[k] = stopped ? rec[k].done : (h[k].frozen ? 0 : s->iters);   // 0 for a frozen instance
            if (reason) reason[k] = stopped ? rec[k].reason : 0;
            if (step) step[k] = rec[k].step;
            if (bound) bound[k] = rec[k].bound;
        }
    })
}

int slp_batch_dga_timing(slp_batch_dga *s, int on) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_batch_dga_timing: NULL handle");
        s->timer.set(on);
    })
}

int slp_batch_dga_timing_read(slp_batch_dga *s, double out[5]) {
    SLP_API_INT({
        SLP_REQUIRE(s && out, "slp_batch_dga_timing_read: NULL argument");
        s->timer.read(out);
    })
}

}  // extern "C"
