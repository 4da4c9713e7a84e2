// slp_cp_batch.hip -- batched Chambolle-Pock: B instances of ONE constraint structure advance per launch.
// No counterpart in the reference (single-threaded numpy: B solves are B calls of chambolle_pock_ppd, ChambollePockPPD.py:36-346).
// The instances share K = [A_eq; A_ineq], hence the preconditioners T, Sigma (:122-179, functions of K and alpha only); they
// differ in c and, optionally, in b, lb, ub, x0.  One iteration = two kernels, as in slp_cp.hip:
//   k_cpb_primal : d = c + K^T y, x+ = clip(x - T d), z = (1+theta) x+ - theta x     [:198-228]
//   k_cpb_dual   : y += Sigma (K z - b), inequality rows clamped at 0                 [:231-240,:333-342]
// Every lane walks its row / column in storage order with a single accumulator (the sums of SLP_ORDER_SEQUENTIAL), so each
// instance is bit for bit the iterate of slp_cp in that order and of the reference, at any row length.
//
// Layout.  Bt = the smallest power of two >= min(B, 64) is the instance-tile width; the batch is padded to
// Bp = Bt * ntiles instances, ntiles = ceil(B / Bt) (one tile for B <= 64, tiles of 64 instances beyond).  A batched
// vector over the n variables is stored tile by tile, the instance index fastest inside a tile:
//   v(j, k)  at  ((k / Bt) * n + j) * Bt + k % Bt          (x, z, x4, c, lb, ub;  y, b with m for n)
// so the Bt values of one variable or row are one contiguous 8 Bt-byte segment (512 B for a full tile) and a tile is
// an independent, contiguous sub-batch.  Padding instances are all zeros (c = lb = ub = b = x = 0): they stay zero and no
// lane ever reads another instance's data.  T[n], Sigma[m] and the CSR pair (K and its device-built transpose) exist once.
//
// Lane mapping.  A workgroup of 256 lanes covers 256 / Bt rows (columns) x Bt instances of the tile blockIdx.y; a wavefront
// 64 / Bt rows x Bt instances.  The Bt lanes of a group read the same row pointer, index and value (with Bt = 64 the row is
// wave-uniform: those loads are scalar) and gather Bt consecutive doubles of y / z per entry.
//
// Report (:242-329), per instance: the row pass forms K x, K x4, K z in one walk (three sequential chains) and the column
// pass c.x, c.x4; row r (column j) belongs to slice r mod S, S = the number of row groups of the launch (<= 1024, a
// function of the shapes only); a slice adds its terms in increasing r, and one lane per instance adds the S slice sums
// in increasing slice order (maxima are exact in any order).  x4 is written by the primal half of a reporting iteration.
//
// Stopping on a certified duality gap, per instance (slp_cp_batch_set_stop_gap, include/slp_hip_ext.h; the certificate of
// slp_cp_many.hip, its scalar arithmetic shared through slp_cp_gap.h).  The state counts its whole iterations t on the host.  From
// the first arming on it launches the MASKED instantiations of k_cpb_primal / k_cpb_dual: the same kernel text, but a lane reads
// stopped[instance] first and returns before any other load.  No barrier anywhere, so a wavefront whose instances are all stopped
// retires at once: with Bt = 64 a wholly stopped tile costs its launch slots only.  Padding instances are marked stopped.
// After the dual half of an iteration t with t % check_every == 0 three launches follow: k_cpb_gap_cols (c.x and the bound's
// column terms, d = c + K^T y by cp_column_sums + cp_direction: the bits of the next primal half), k_cpb_gap_rows (the y.b
// terms and the two violation maxima, K x one accumulator in storage order) -- both sliced as the report's passes (entry r in
// slice r mod S, a slice in increasing r), in rowparts / colparts, which are free between reports on the one stream; a batch of
// fewer than 256 instances gets up to 4096 slices, in scratch allocated at the first arming (kCpbGapLanes) -- and k_cpb_gap_final, one lane per running instance and quantity: the slice
// sums in increasing slice order, the decision, the record, the flag, and a device count of the instances that go on.  Nothing is
// read back while iterations are enqueued; an armed iterate / dual_step begins with one read of that count and enqueues
// nothing when it is 0.  One counter for the whole batch: a stopped instance stays stopped for the life of the state.
#include <cmath>
#include <vector>

#include "../../include/slp_hip_ext.h"
#include "slp_common.h"
#include "slp_cp_gap.h"
#include "slp_cp_shared.h"
#include "slp_kernels.h"

namespace slp {

// slp_cp.hip: T and Sigma by the CSR walks of the single-instance set-up
void cp_preconditioners_csr(slp_matrix *k, i64 m_eq, double alpha, double *t, double *sigma);

constexpr int kCpbMaxSlices = 1024;
// the certificate's passes: with 1024 slices a batch of one tile fills an eighth of the device's wave slots and a pass is a chain of
// memory latencies (measured: DESIGN.md section 7), so a narrow batch gets up to 4096 slices in scratch of the test's own --
// kCpbGapLanes lanes per pass where the batch allows; a batch of 256 or more instances keeps the report's 1024 and its scratch
constexpr int kCpbGapMaxSlices = 4096;
constexpr i64 kCpbGapLanes = 262144;
constexpr int kCpbGapAhead = 16;

// the row (column) a lane group works on; with a full tile it is the same for the whole wavefront: scalar registers
template <int BT>
__device__ __forceinline__ i64 cpb_uniform(i64 v) {
    if (BT == kWave) {
        const unsigned int lo = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(unsigned long long)v);
        const unsigned int hi = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)((unsigned long long)v >> 32));
        return (i64)(((unsigned long long)hi << 32) | lo);
    }
    return v;
}

// host [B x len] (or one shared [len] vector) -> the tiled layout; padding instances are zero
__global__ void k_cpb_scatter(i64 len, i64 B, int BT, i64 Bp, const double *__restrict__ src, int batched, double *__restrict__ dst) {
    const i64 total = len * Bp;
    for (i64 o = (i64)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (i64)gridDim.x * blockDim.x) {
        const i64 k = o % BT, rest = o / BT, j = rest % len, tile = rest / len;
        const i64 inst = tile * BT + k;
        dst[o] = inst < B ? src[batched ? inst * len + j : j] : 0.0;
    }
}

// the tiled layout -> [B x len], row-major
__global__ void k_cpb_gather(i64 len, i64 B, int BT, const double *__restrict__ src, double *__restrict__ dst) {
    const i64 total = len * B;
    for (i64 o = (i64)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (i64)gridDim.x * blockDim.x) {
        const i64 inst = o / len, j = o - inst * len;
        dst[o] = src[((inst / BT) * len + j) * BT + inst % BT];
    }
}

// primal half-iteration: one lane per (column j, instance k); STORE: also x4_j = ub_j if d_j < 0 else lb_j (:260-261).
// MASKED, for a state with stopped instances: a lane reads its instance's flag first and returns before any other load;
// `stopped` is not looked at without it.
template <int BT, bool STORE, bool MASKED>
__global__ __launch_bounds__(kBlock) void k_cpb_primal(i64 n, i64 m, const i64 *__restrict__ tptr, const i32 *__restrict__ tidx,
                                                       const double *__restrict__ tval, const double *__restrict__ y,
                                                       const double *__restrict__ c, const double *__restrict__ t,
                                                       const double *__restrict__ lb, const double *__restrict__ ub,
                                                       double *__restrict__ x, double *__restrict__ z, double *__restrict__ x4,
                                                       i32 m_eq, i64 m_ineq, double one_plus_theta, double theta,
                                                       const i32 *__restrict__ stopped) {
    const int k = threadIdx.x & (BT - 1);
    const i64 tile = blockIdx.y;
    if (MASKED && stopped[tile * BT + k]) return;
    const i64 group = ((i64)blockIdx.x * kBlock + threadIdx.x) / BT;
    const i64 ngroups = (i64)gridDim.x * kBlock / BT;
    const double *__restrict__ yt = y + tile * m * BT + k;
    for (i64 jj = group; jj < n; jj += ngroups) {
        const i64 j = cpb_uniform<BT>(jj);  // MASKED: the first ACTIVE lane's; every lane of the wave has the same column
        const i64 s = tptr[j], e = tptr[j + 1];
        // storage order, equality and inequality partial sums apart (slp_cp_shared.h: the set solver runs the same functions)
        double se, si;
        cp_column_sums(s, e, tidx, tval, yt, BT, m_eq, CpLoadPlain(), &se, &si);
        const i64 o = (tile * n + j) * BT + k;
        const double d = cp_direction(c[o], se, si, m_eq > 0, m_ineq > 0);  // :206,216
        const double xo = x[o], l = lb[o], u = ub[o];
        double x2, zn;
        cp_primal_point(d, xo, t[j], l, u, one_plus_theta, theta, &x2, &zn);  // :220,226
        z[o] = zn;
        x[o] = x2;
        if (STORE) x4[o] = (d < 0.0) ? u : l;
    }
}

// dual half-iteration: one lane per (row i, instance k); MASKED as in k_cpb_primal
template <int BT, bool MASKED>
__global__ __launch_bounds__(kBlock) void k_cpb_dual(i64 n, i64 m, const i64 *__restrict__ ptr, const i32 *__restrict__ idx,
                                                     const double *__restrict__ val, const double *__restrict__ z,
                                                     const double *__restrict__ b, const double *__restrict__ sigma,
                                                     double *__restrict__ y, i64 m_eq, const i32 *__restrict__ stopped) {
    const int k = threadIdx.x & (BT - 1);
    const i64 tile = blockIdx.y;
    if (MASKED && stopped[tile * BT + k]) return;
    const i64 group = ((i64)blockIdx.x * kBlock + threadIdx.x) / BT;
    const i64 ngroups = (i64)gridDim.x * kBlock / BT;
    const double *__restrict__ zt = z + tile * n * BT + k;
    for (i64 ii = group; ii < m; ii += ngroups) {
        const i64 i = cpb_uniform<BT>(ii);
        const i64 s = ptr[i], e = ptr[i + 1];
        const double kz = cp_row_sum(s, e, idx, val, zt, BT, CpLoadPlain());
        const i64 o = (tile * m + i) * BT + k;
        y[o] = cp_dual_point(kz, b[o], y[o], sigma[i], i >= m_eq);  // :235,240,:334,339,:341
    }
}

// report, row pass.  part[(q * S + slice) * Bp + instance], S = gridDim.x * 256 / BT slices:
//   q = 0 sum y_i (Kx - b)_i   1 sum y_i (Kx4 - b)_i   2 max_{i<m_eq} |Kz - b|   3 max_{i>=m_eq} (Kx - b)   4 max_{i<m_eq} |Kx - b|
template <int BT>
__global__ __launch_bounds__(kBlock) void k_cpb_report_rows(i64 n, i64 m, const i64 *__restrict__ ptr, const i32 *__restrict__ idx,
                                                            const double *__restrict__ val, const double *__restrict__ x,
                                                            const double *__restrict__ x4, const double *__restrict__ z,
                                                            const double *__restrict__ b, const double *__restrict__ y, i64 m_eq,
                                                            i64 Bp, double *__restrict__ part) {
    const int k = threadIdx.x & (BT - 1);
    const i64 tile = blockIdx.y;
    const i64 group = ((i64)blockIdx.x * kBlock + threadIdx.x) / BT;
    const i64 ngroups = (i64)gridDim.x * kBlock / BT;
    const i64 vo = tile * n * BT + k;
    double s1 = 0.0, s2 = 0.0, veq = -__builtin_inf(), vin = -__builtin_inf(), veqx = -__builtin_inf();
    for (i64 ii = group; ii < m; ii += ngroups) {
        const i64 i = cpb_uniform<BT>(ii);
        double kx = 0.0, kx4 = 0.0, kz = 0.0;  // three chains in storage order
        for (i64 q = ptr[i]; q < ptr[i + 1]; ++q) {
            const i64 at = vo + (i64)idx[q] * BT;
            const double a = val[q];
            kx += a * x[at];
            kx4 += a * x4[at];
            kz += a * z[at];
        }
        const i64 o = (tile * m + i) * BT + k;
        const double bi = b[o], yi = y[o];
        s1 += yi * (kx - bi);
        s2 += yi * (kx4 - bi);
        if (i < m_eq) {
            const double a = fabs(kz - bi), ax = fabs(kx - bi);
            veq = a > veq ? a : veq;
            veqx = ax > veqx ? ax : veqx;
        } else {
            const double v = kx - bi;
            vin = v > vin ? v : vin;
        }
    }
    const i64 inst = tile * BT + k;
    part[(0 * ngroups + group) * Bp + inst] = s1;
    part[(1 * ngroups + group) * Bp + inst] = s2;
    part[(2 * ngroups + group) * Bp + inst] = veq;
    part[(3 * ngroups + group) * Bp + inst] = vin;
    part[(4 * ngroups + group) * Bp + inst] = veqx;
}

// report, column pass.  part[(q * S + slice) * Bp + instance]: q = 0 sum c x, 1 sum c x4
template <int BT>
__global__ __launch_bounds__(kBlock) void k_cpb_report_cols(i64 n, const double *__restrict__ c, const double *__restrict__ x,
                                                            const double *__restrict__ x4, i64 Bp, double *__restrict__ part) {
    const int k = threadIdx.x & (BT - 1);
    const i64 tile = blockIdx.y;
    const i64 group = ((i64)blockIdx.x * kBlock + threadIdx.x) / BT;
    const i64 ngroups = (i64)gridDim.x * kBlock / BT;
    double s0 = 0.0, s1 = 0.0;
    for (i64 j = group; j < n; j += ngroups) {
        const i64 o = (tile * n + j) * BT + k;
        const double cj = c[o];
        s0 += cj * x[o];
        s1 += cj * x4[o];
    }
    const i64 inst = tile * BT + k;
    part[(0 * ngroups + group) * Bp + inst] = s0;
    part[(1 * ngroups + group) * Bp + inst] = s1;
}

// one lane per instance: the slice sums in increasing slice order; out[inst * 5 + 0..4] as slp_cp_report
__global__ void k_cpb_report_final(i64 Bp, i64 srows, const double *__restrict__ rp, i64 scols, const double *__restrict__ cp, i64 m_eq,
                                   double *__restrict__ out) {
    const i64 inst = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (inst >= Bp) return;
    double s1 = 0.0, s2 = 0.0, veq = -__builtin_inf(), vin = -__builtin_inf(), veqx = -__builtin_inf(), c0 = 0.0, c1 = 0.0;
    for (i64 g = 0; g < srows; ++g) {
        s1 += rp[(0 * srows + g) * Bp + inst];
        s2 += rp[(1 * srows + g) * Bp + inst];
        const double a = rp[(2 * srows + g) * Bp + inst], v = rp[(3 * srows + g) * Bp + inst], ax = rp[(4 * srows + g) * Bp + inst];
        veq = a > veq ? a : veq;
        vin = v > vin ? v : vin;
        veqx = ax > veqx ? ax : veqx;
    }
    for (i64 g = 0; g < scols; ++g) {
        c0 += cp[(0 * scols + g) * Bp + inst];
        c1 += cp[(1 * scols + g) * Bp + inst];
    }
    out[inst * 5 + 0] = c0 + s1;
    out[inst * 5 + 1] = c1 + s2;
    out[inst * 5 + 2] = (m_eq > 0) ? (veq == -__builtin_inf() ? 0.0 : veq) : 0.0;
    out[inst * 5 + 3] = vin;
    out[inst * 5 + 4] = (veqx == -__builtin_inf()) ? 0.0 : veqx;
}

// ---- per-instance stopping on a certified duality gap (header comment; slp_cp_batch_set_stop_gap) ----
// The arithmetic per column, per row and of the decision is slp_cp_gap.h's; an armed state iterates with MASKED.

// certificate, column pass (the report's slices).  part[(q * S + slice) * Bp + instance]: q = 0 sum c_j x_j, 1 the bound's column
// terms sum [d_j != 0 ? min(d_j lb_j, d_j ub_j) : 0] with d = c + K^T y as the next primal half forms it
template <int BT>
__global__ __launch_bounds__(kBlock) void k_cpb_gap_cols(i64 n, i64 m, const i64 *__restrict__ tptr, const i32 *__restrict__ tidx,
                                                         const double *__restrict__ tval, const double *__restrict__ y,
                                                         const double *__restrict__ c, const double *__restrict__ lb,
                                                         const double *__restrict__ ub, const double *__restrict__ x, i32 m_eq, i64 m_ineq,
                                                         i64 Bp, const i32 *__restrict__ stopped, double *__restrict__ part) {
    const int k = threadIdx.x & (BT - 1);
    const i64 tile = blockIdx.y;
    const i64 inst = tile * BT + k;
    if (stopped[inst]) return;
    const i64 group = ((i64)blockIdx.x * kBlock + threadIdx.x) / BT;
    const i64 ngroups = (i64)gridDim.x * kBlock / BT;
    const double *__restrict__ yt = y + tile * m * BT + k;
    double cx = 0.0, terms = 0.0;
    for (i64 jj = group; jj < n; jj += ngroups) {
        const i64 j = cpb_uniform<BT>(jj);
        double se, si;
        cp_column_sums(tptr[j], tptr[j + 1], tidx, tval, yt, BT, m_eq, CpLoadPlain(), &se, &si);
        const i64 o = (tile * n + j) * BT + k;
        const double cj = c[o];
        const double d = cp_direction(cj, se, si, m_eq > 0, m_ineq > 0);
        cx += cj * x[o];
        terms += cp_gap_col_term(d, lb[o], ub[o]);
    }
    part[(0 * ngroups + group) * Bp + inst] = cx;
    part[(1 * ngroups + group) * Bp + inst] = terms;
}

// certificate, row pass.  part[(q * S + slice) * Bp + instance]: q = 0 sum [y_r != 0 ? y_r b_r : 0],
// 1 max_{r < m_eq} |(K x)_r - b_r| and 2 max_{r >= m_eq} ((K x)_r - b_r), each with 0 (K x: one accumulator in storage order)
template <int BT>
__global__ __launch_bounds__(kBlock) void k_cpb_gap_rows(i64 n, i64 m, const i64 *__restrict__ ptr, const i32 *__restrict__ idx,
                                                         const double *__restrict__ val, const double *__restrict__ x,
                                                         const double *__restrict__ b, const double *__restrict__ y, i64 m_eq, i64 Bp,
                                                         const i32 *__restrict__ stopped, double *__restrict__ part) {
    const int k = threadIdx.x & (BT - 1);
    const i64 tile = blockIdx.y;
    const i64 inst = tile * BT + k;
    if (stopped[inst]) return;
    const i64 group = ((i64)blockIdx.x * kBlock + threadIdx.x) / BT;
    const i64 ngroups = (i64)gridDim.x * kBlock / BT;
    const double *__restrict__ xt = x + tile * n * BT + k;
    double yb = 0.0, veq = 0.0, vin = 0.0;
    for (i64 ii = group; ii < m; ii += ngroups) {
        const i64 i = cpb_uniform<BT>(ii);
        const double kx = cp_row_sum(ptr[i], ptr[i + 1], idx, val, xt, BT, CpLoadPlain());
        const i64 o = (tile * m + i) * BT + k;
        const double bi = b[o];
        yb += cp_gap_row_term(y[o], bi);
        if (i < m_eq) veq = cp_gap_violation(veq, kx - bi, true);
        else vin = cp_gap_violation(vin, kx - bi, false);
    }
    part[(0 * ngroups + group) * Bp + inst] = yb;
    part[(1 * ngroups + group) * Bp + inst] = veq;
    part[(2 * ngroups + group) * Bp + inst] = vin;
}

// one workgroup of five wavefronts per 64 instances, wavefront q folding quantity q of a running real instance over the slices in
// increasing slice order (q = 0 sum y b, 1 and 2 the violation maxima: the row pass; 3 c.x, 4 the bound's column terms: the
// column pass), kCpbGapAhead slices loaded before they are added; behind the barrier wavefront 0 decides and writes the record
// rec[3 inst + 0..2] = primal, bound, violation, the flag with the stopping iteration `t`, and counts the instances that go on
// (`running` is zeroed on the stream before this launch).  Every lane reaches the barrier.
constexpr int kCpbGapQuantities = 5;
__global__ __launch_bounds__(kCpbGapQuantities *kWave) void k_cpb_gap_final(i64 B, i64 Bp, i64 srows, const double *__restrict__ rp, i64 scols,
                                                                            const double *__restrict__ cp, double tol_gap, double tol_feas,
                                                                            i64 t, i32 *__restrict__ stopped, i64 *__restrict__ stop_iter,
                                                                            double *__restrict__ rec, i32 *__restrict__ running) {
    __shared__ double folded[kCpbGapQuantities][kWave];
    const int q = (int)threadIdx.x / kWave, lane = (int)threadIdx.x % kWave;
    const i64 inst = (i64)blockIdx.x * kWave + lane;
    const bool live = inst < B && !stopped[inst];
    double acc = 0.0;
    if (live) {
        const bool rows = q < 3, is_max = q == 1 || q == 2;
        const i64 S = rows ? srows : scols;
        const double *__restrict__ p = (rows ? rp + (i64)q * srows * Bp : cp + (i64)(q - 3) * scols * Bp) + inst;
        for (i64 g0 = 0; g0 < S; g0 += kCpbGapAhead) {
            double a[kCpbGapAhead];
#pragma unroll
            for (int u = 0; u < kCpbGapAhead; ++u) {
                const i64 g = (g0 + u < S) ? g0 + u : S - 1;
                a[u] = p[g * Bp];
            }
#pragma unroll
            for (int u = 0; u < kCpbGapAhead; ++u)
                if (g0 + u < S) acc = is_max ? nan_max(acc, a[u]) : acc + a[u];
        }
    }
    folded[q][lane] = acc;
    __syncthreads();
    if (q != 0 || !live) return;
    const double viol = nan_max(folded[1][lane], folded[2][lane]), primal = folded[3][lane];
    double bound;
    const bool stop = cp_gap_decide(primal, folded[4][lane], folded[0][lane], viol, tol_gap, tol_feas, &bound);
    rec[inst * 3 + 0] = primal;
    rec[inst * 3 + 1] = bound;
    rec[inst * 3 + 2] = viol;
    if (stop) {
        stopped[inst] = 1;
        stop_iter[inst] = t;
    } else {
        atomicAdd(running, 1);
    }
}

}  // namespace slp

using namespace slp;

struct slp_cp_batch {
    slp_matrix *k = nullptr;  // owned
    i64 n = 0, m = 0, m_eq = 0, m_ineq = 0;
    i64 B = 0, Bp = 0, ntiles = 0;
    int Bt = 1;
    double alpha = 1, theta = 1;
    DevBuf<double> b, c, lb, ub, t, sigma, x, z, y, x4, rowparts, colparts, out;
    i64 iters = 0;  // whole iterations over the state's life: bumped where a dual half is enqueued
    // the certificate test (slp_cp_batch_set_stop_gap); its buffers exist from the first arming on, and from then on the state
    // launches the MASKED kernels.  Off while tol_gap < 0.
    bool masked = false;
    double tol_gap = -1.0, tol_feas = 0.0;
    i64 check_every = 1;
    DevBuf<i32> stopped, running;  // per padded instance; the count of real instances that still run
    DevBuf<i64> stop_iter;
    DevBuf<double> rec;  // primal, bound, violation of the last evaluated certificate, per instance
    i64 gap_slices = kCpbMaxSlices;  // at most this many slices per certificate pass
    DevBuf<double> gapparts;         // 5 * gap_slices * Bp slice sums where gap_slices exceeds the report's
    ~slp_cp_batch() { delete k; }
};

namespace slp {

// Dispatch a kernel template on the instance-tile width.
#define SLP_DISPATCH_TILE(bt, CALL)                        \
    switch (bt) {                                          \
        case 1:  { constexpr int BT = 1;  CALL; } break;   \
        case 2:  { constexpr int BT = 2;  CALL; } break;   \
        case 4:  { constexpr int BT = 4;  CALL; } break;   \
        case 8:  { constexpr int BT = 8;  CALL; } break;   \
        case 16: { constexpr int BT = 16; CALL; } break;   \
        case 32: { constexpr int BT = 32; CALL; } break;   \
        default: { constexpr int BT = 64; CALL; } break;   \
    }

static dim3 cpb_grid(const slp_cp_batch *s, i64 rows) { return dim3((unsigned)grid_for(rows * s->Bt, kBlock), (unsigned)s->ntiles); }

// blocks of a sliced pass (the report's: kCpbMaxSlices; the certificate's: s->gap_slices): at most `max_slices` row groups
static dim3 cpb_slice_grid(const slp_cp_batch *s, i64 rows, i64 max_slices) {
    const i64 per_block = kBlock / s->Bt;
    i64 g = (rows + per_block - 1) / per_block;
    const i64 cap = std::max<i64>(1, max_slices / per_block);
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return dim3((unsigned)g, (unsigned)s->ntiles);
}

template <bool STORE, bool MASKED>
static void cpb_launch_primal(slp_cp_batch *s) {
    const CsrDev &at = s->k->at;
    SLP_DISPATCH_TILE(s->Bt, hipLaunchKernelGGL((k_cpb_primal<BT, STORE, MASKED>), cpb_grid(s, s->n), dim3(kBlock), 0, ctx().stream, s->n, s->m,
                                                at.ptr.p, at.idx.p, at.val.p, s->y.p, s->c.p, s->t.p, s->lb.p, s->ub.p, s->x.p, s->z.p, s->x4.p,
                                                (i32)s->m_eq, s->m_ineq, 1.0 + s->theta, s->theta, s->stopped.p));
    SLP_HIP(hipGetLastError());
}

static void cpb_primal(slp_cp_batch *s, bool store) {
    if (s->masked) store ? cpb_launch_primal<true, true>(s) : cpb_launch_primal<false, true>(s);
    else store ? cpb_launch_primal<true, false>(s) : cpb_launch_primal<false, false>(s);
}

template <bool MASKED>
static void cpb_launch_dual(slp_cp_batch *s) {
    const CsrDev &a = s->k->a;
    SLP_DISPATCH_TILE(s->Bt, hipLaunchKernelGGL((k_cpb_dual<BT, MASKED>), cpb_grid(s, s->m), dim3(kBlock), 0, ctx().stream, s->n, s->m, a.ptr.p,
                                                a.idx.p, a.val.p, s->z.p, s->b.p, s->sigma.p, s->y.p, s->m_eq, s->stopped.p));
    SLP_HIP(hipGetLastError());
}

static void cpb_dual(slp_cp_batch *s) {
    s->masked ? cpb_launch_dual<true>(s) : cpb_launch_dual<false>(s);
    ++s->iters;  // the dual half ends an iteration
}

// the certificate of iteration s->iters for every running instance, enqueued behind its dual half; nothing is read back
static void cpb_certificate(slp_cp_batch *s) {
    hipStream_t st = ctx().stream;
    const CsrDev &a = s->k->a, &at = s->k->at;
    const dim3 gr = cpb_slice_grid(s, s->m, s->gap_slices), gc = cpb_slice_grid(s, s->n, s->gap_slices);
    const i64 srows = (i64)gr.x * kBlock / s->Bt, scols = (i64)gc.x * kBlock / s->Bt;
    // 3 * srows * Bp and 2 * scols * Bp slice sums: the report's scratch holds 5 and 2 times 1024 * Bp
    const bool own = s->gap_slices > kCpbMaxSlices;
    double *rowparts = own ? s->gapparts.p : s->rowparts.p;
    double *colparts = own ? s->gapparts.p + (size_t)3 * (size_t)s->gap_slices * (size_t)s->Bp : s->colparts.p;
    SLP_DISPATCH_TILE(s->Bt, hipLaunchKernelGGL((k_cpb_gap_cols<BT>), gc, dim3(kBlock), 0, st, s->n, s->m, at.ptr.p, at.idx.p, at.val.p,
                                                s->y.p, s->c.p, s->lb.p, s->ub.p, s->x.p, (i32)s->m_eq, s->m_ineq, s->Bp, s->stopped.p,
                                                colparts));
    SLP_HIP(hipGetLastError());
    SLP_DISPATCH_TILE(s->Bt, hipLaunchKernelGGL((k_cpb_gap_rows<BT>), gr, dim3(kBlock), 0, st, s->n, s->m, a.ptr.p, a.idx.p, a.val.p,
                                                s->x.p, s->b.p, s->y.p, s->m_eq, s->Bp, s->stopped.p, rowparts));
    SLP_HIP(hipGetLastError());
    s->running.zero();
    hipLaunchKernelGGL(k_cpb_gap_final, dim3((unsigned)((s->B + kWave - 1) / kWave)), dim3(kCpbGapQuantities * kWave), 0, st, s->B, s->Bp, srows,
                       rowparts, scols, colparts, s->tol_gap, s->tol_feas, s->iters, s->stopped.p, s->stop_iter.p, s->rec.p,
                       s->running.p);
    SLP_HIP(hipGetLastError());
}

// an armed state asks once per call whether anything is left to run
static bool cpb_all_stopped(slp_cp_batch *s) {
    if (!s->masked) return false;
    i32 running = 0;
    s->running.download(&running, 1);
    return running == 0;
}

// whole iterations; the host knows the count, so it knows where the certificate is due
static void cpb_iterations(slp_cp_batch *s, i64 k, bool with_primal) {
    if (cpb_all_stopped(s)) return;
    for (i64 it = 0; it < k; ++it) {
        if (with_primal) cpb_primal(s, false);
        cpb_dual(s);
        if (s->tol_gap >= 0.0 && s->iters % s->check_every == 0) cpb_certificate(s);
    }
}

// host vector(s) -> tiled device layout through `stage`
static void cpb_upload(slp_cp_batch *s, DevBuf<double> &stage, const double *host, int batched, i64 len, DevBuf<double> &dst) {
    hipStream_t st = ctx().stream;
    const size_t count = (size_t)len * (size_t)(batched ? s->B : 1);
    SLP_HIP(hipMemcpyAsync(stage.p, host, count * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_cpb_scatter, dim3(grid_for(len * s->Bp, kBlock)), dim3(kBlock), 0, st, len, s->B, s->Bt, s->Bp, stage.p, batched,
                       dst.p);
    SLP_HIP(hipGetLastError());
    SLP_HIP(hipStreamSynchronize(st));  // the host buffer may be freed by the caller; the stage is reused
}

static void cpb_download(slp_cp_batch *s, const DevBuf<double> &src, i64 len, double *host) {
    hipStream_t st = ctx().stream;
    DevBuf<double> stage((size_t)len * (size_t)s->B);
    hipLaunchKernelGGL(k_cpb_gather, dim3(grid_for(len * s->B, kBlock)), dim3(kBlock), 0, st, len, s->B, s->Bt, src.p, stage.p);
    SLP_HIP(hipGetLastError());
    stage.download(host, (size_t)len * (size_t)s->B);
}

}  // namespace slp

extern "C" {

slp_cp_batch *slp_cp_batch_create(int64_t n, int64_t m_eq, int64_t m_ineq, const int64_t *indptr, const int32_t *indices,
                                  const double *data, int64_t batch, const double *b, int b_batched, const double *c,
                                  const double *lb, int lb_batched, const double *ub, int ub_batched, const double *x0,
                                  int x0_batched, double alpha, double theta) {
    SLP_API_PTR({
        SLP_REQUIRE(indptr && b && c && lb && ub, "slp_cp_batch_create: NULL argument");
        SLP_REQUIRE(n >= 1 && m_eq >= 0 && m_ineq >= 0 && m_eq + m_ineq >= 1, "slp_cp_batch_create: needs at least one variable and one row");
        SLP_REQUIRE(batch >= 1, "slp_cp_batch_create: batch must be at least 1");
        const i64 m = m_eq + m_ineq, nnz = indptr[m];
        SLP_REQUIRE(nnz >= 0, "slp_cp_batch_create: indptr must be non-decreasing");
        int bt = 1;
        while (bt < kWave && bt < batch) bt *= 2;
        const double ntiles = (double)((batch - 1) / bt + 1), bp = ntiles * bt;
        // nothing is allocated, and no batched argument is read, before this check: the CSR pair and the scratch of the device
        // transposition, the eight batched vectors (x, z, x4, c, lb, ub over n; y, b over m), the staging buffer of one host
        // vector, T and Sigma, the report's slice sums
        {
            i64 free_b = 0, total_b = 0;
            SLP_REQUIRE(slp_device_memory(&free_b, &total_b) == 0, slp_last_error());
            const double vectors = (6.0 * (double)n + 2.0 * (double)m) * 8.0 * bp;
            const double need = 40.0 * (double)nnz + 16.0 * (double)(n + m + 2) + vectors + 8.0 * (double)std::max(n, m) * (double)batch +
                                8.0 * (double)(n + m) + 8.0 * (7.0 * kCpbMaxSlices + 5.0) * bp;
            const double have = (double)free_b + (double)slp_cached_bytes();
            if (need > have)
                throw Error("slp_cp_batch_create: " + std::to_string(batch) + " instances need " + std::to_string(need / 1e9) +
                            " GB of device memory (batched vectors: " + std::to_string(vectors / 1e9) + " GB), " +
                            std::to_string(have / 1e9) + " GB are free");
        }
        SLP_REQUIRE(ntiles <= 65535.0, "slp_cp_batch_create: at most 65535 tiles of 64 instances");
        slp_matrix *k = slp_matrix_create(m, n, indptr, indices, data);  // validates the column indices
        if (!k) throw Error(slp_last_error());
        auto *s = new slp_cp_batch();
        s->k = k;
        try {
            s->n = n; s->m = m; s->m_eq = m_eq; s->m_ineq = m_ineq;
            s->B = batch; s->Bt = bt; s->ntiles = (i64)ntiles; s->Bp = s->ntiles * bt;
            s->alpha = alpha; s->theta = theta;
            require_csr(k, "slp_cp_batch_create");  // the batch iterates on the CSR pair only
            build_transpose(k);
            s->t.alloc((size_t)n);
            s->sigma.alloc((size_t)m);
            cp_preconditioners_csr(k, m_eq, alpha, s->t.p, s->sigma.p);
            const size_t nb = (size_t)n * (size_t)s->Bp, mb = (size_t)m * (size_t)s->Bp;
            s->c.alloc(nb); s->lb.alloc(nb); s->ub.alloc(nb); s->x.alloc(nb); s->z.alloc(nb); s->x4.alloc(nb);
            s->b.alloc(mb); s->y.alloc(mb);
            s->rowparts.alloc((size_t)5 * kCpbMaxSlices * (size_t)s->Bp);
            s->colparts.alloc((size_t)2 * kCpbMaxSlices * (size_t)s->Bp);
            s->out.alloc((size_t)5 * (size_t)s->Bp);
            {
                DevBuf<double> stage((size_t)std::max(n, m) * (size_t)batch);
                cpb_upload(s, stage, c, 1, n, s->c);
                cpb_upload(s, stage, lb, lb_batched, n, s->lb);
                cpb_upload(s, stage, ub, ub_batched, n, s->ub);
                cpb_upload(s, stage, b, b_batched, m, s->b);
                if (x0) cpb_upload(s, stage, x0, x0_batched, n, s->x);
                else s->x.zero();
            }
            s->z.copy_from(s->x);  // x3 = x (:190)
            s->y.zero();           // :166,177
            s->x4.zero();
            SLP_HIP(hipStreamSynchronize(ctx().stream));
        } catch (...) {
            delete s;
            throw;
        }
        return s;
    })
}

void slp_cp_batch_destroy(slp_cp_batch *s) { delete s; }

int slp_cp_batch_iterate(slp_cp_batch *s, int64_t k) {
    SLP_API_INT({
        SLP_REQUIRE(s && k >= 0, "slp_cp_batch_iterate: bad arguments");
        cpb_iterations(s, k, true);
    })
}

int slp_cp_batch_primal_step(slp_cp_batch *s) { SLP_API_INT({ SLP_REQUIRE(s, "NULL handle"); cpb_primal(s, true); }) }

int slp_cp_batch_dual_step(slp_cp_batch *s) { SLP_API_INT({ SLP_REQUIRE(s, "NULL handle"); cpb_iterations(s, 1, false); }) }

int slp_cp_batch_report(slp_cp_batch *s, double *out) {
    SLP_API_INT({
        SLP_REQUIRE(s && out, "slp_cp_batch_report: NULL argument");
        hipStream_t st = ctx().stream;
        const CsrDev &a = s->k->a;
        const dim3 gr = cpb_slice_grid(s, s->m, kCpbMaxSlices), gc = cpb_slice_grid(s, s->n, kCpbMaxSlices);
        const i64 srows = (i64)gr.x * kBlock / s->Bt, scols = (i64)gc.x * kBlock / s->Bt;
        SLP_DISPATCH_TILE(s->Bt, hipLaunchKernelGGL((k_cpb_report_cols<BT>), gc, dim3(kBlock), 0, st, s->n, s->c.p, s->x.p, s->x4.p, s->Bp,
                                                    s->colparts.p));
        SLP_HIP(hipGetLastError());
        SLP_DISPATCH_TILE(s->Bt, hipLaunchKernelGGL((k_cpb_report_rows<BT>), gr, dim3(kBlock), 0, st, s->n, s->m, a.ptr.p, a.idx.p, a.val.p,
                                                    s->x.p, s->x4.p, s->z.p, s->b.p, s->y.p, s->m_eq, s->Bp, s->rowparts.p));
        SLP_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_cpb_report_final, dim3((unsigned)((s->Bp + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, s->Bp, srows,
                           s->rowparts.p, scols, s->colparts.p, s->m_eq, s->out.p);
        SLP_HIP(hipGetLastError());
        s->out.download(out, (size_t)5 * (size_t)s->B);  // instance k at out[5 k]: the padding instances come last
    })
}

int slp_cp_batch_get_x(slp_cp_batch *s, double *x) { SLP_API_INT({ SLP_REQUIRE(s && x, "NULL argument"); cpb_download(s, s->x, s->n, x); }) }

int slp_cp_batch_get_y(slp_cp_batch *s, double *y) { SLP_API_INT({ SLP_REQUIRE(s && y, "NULL argument"); cpb_download(s, s->y, s->m, y); }) }

int slp_cp_batch_get_preconditioners(slp_cp_batch *s, double *t, double *sigma) {
    SLP_API_INT({
        SLP_REQUIRE(s, "NULL handle");
        if (t) s->t.download(t, (size_t)s->n);
        if (sigma) s->sigma.download(sigma, (size_t)s->m);
    })
}

int slp_cp_batch_bench(slp_cp_batch *s, int64_t k, double ms[3]) {
    SLP_API_INT({
        SLP_REQUIRE(s && k > 0 && ms, "slp_cp_batch_bench: bad arguments");
        Context &c = ctx();
        // milliseconds per repetition of `k` times the halves in `stages` (bit 0 primal, bit 1 dual)
        auto timed = [&](int stages) {
            float f = 0.f;
            SLP_HIP(hipEventRecord(c.ev0, c.stream));
            for (i64 it = 0; it < k; ++it) {
                if (stages & 1) cpb_primal(s, false);
                if (stages & 2) cpb_dual(s);
            }
            SLP_HIP(hipEventRecord(c.ev1, c.stream));
            SLP_HIP(hipEventSynchronize(c.ev1));
            SLP_HIP(hipEventElapsedTime(&f, c.ev0, c.ev1));
            return (double)f / (double)k;
        };
        ms[0] = timed(3);
        ms[1] = timed(1);
        ms[2] = timed(2);
    })
}

int slp_cp_batch_set_stop_gap(slp_cp_batch *s, double tol_gap, double tol_feas, int64_t check_every) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_cp_batch_set_stop_gap: NULL handle");
        SLP_REQUIRE(tol_gap < 0.0 || (std::isfinite(tol_gap) && std::isfinite(tol_feas) && tol_feas >= 0.0 && check_every >= 1),
                    "slp_cp_batch_set_stop_gap: tol_gap and tol_feas must be finite and >= 0 with check_every >= 1 (tol_gap < 0 turns the "
                    "test off)");
        if (tol_gap >= 0.0 && !s->masked) {  // the first arming: flags (padding instances stopped), records, the count
            const size_t bp = (size_t)s->Bp;
            std::vector<i32> flags(bp, 0);
            for (size_t k = (size_t)s->B; k < bp; ++k) flags[k] = 1;
            std::vector<double> rec(3 * bp);
            for (size_t k = 0; k < bp; ++k) {
                rec[3 * k + 0] = __builtin_inf();
                rec[3 * k + 1] = -__builtin_inf();
                rec[3 * k + 2] = __builtin_inf();
            }
            const std::vector<i64> none(bp, 0);
            const i32 running = (i32)std::min<i64>(s->B, 0x7fffffff);
            const i64 slices = std::min<i64>(kCpbGapMaxSlices, std::max<i64>(kCpbMaxSlices, kCpbGapLanes / s->Bp));
            if (slices > kCpbMaxSlices) s->gapparts.alloc((size_t)5 * (size_t)slices * bp);
            s->gap_slices = slices;
            s->stopped.upload(flags.data(), bp);
            s->stop_iter.upload(none.data(), bp);
            s->rec.upload(rec.data(), 3 * bp);
            s->running.upload(&running, 1);
            s->masked = true;
        }
        s->tol_gap = tol_gap < 0.0 ? -1.0 : tol_gap;
        if (tol_gap >= 0.0) {
            s->tol_feas = tol_feas;
            s->check_every = check_every;
        }
    })
}

int slp_cp_batch_gap_state(slp_cp_batch *s, int64_t *iterations, int32_t *stopped, double *primal, double *bound, double *violation) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_cp_batch_gap_state: NULL handle");
        const size_t count = (size_t)s->B;
        std::vector<i32> flags(count, 0);
        std::vector<i64> at(count, 0);
        std::vector<double> rec(3 * count);
        if (s->masked) {
            s->stopped.download(flags.data(), count);
            s->stop_iter.download(at.data(), count);
            s->rec.download(rec.data(), 3 * count);
        }
        for (size_t k = 0; k < count; ++k) {
            if (iterations) iterations[k] = flags[k] ? at[k] : s->iters;
            if (stopped) stopped[k] = flags[k];
            if (primal) primal[k] = s->masked ? rec[3 * k + 0] : __builtin_inf();
            if (bound) bound[k] = s->masked ? rec[3 * k + 1] : -__builtin_inf();
            if (violation) violation[k] = s->masked ? rec[3 * k + 2] : __builtin_inf();
        }
    })
}

}  // extern "C"
