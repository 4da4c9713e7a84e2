// slp_gap_fold.h -- the slice count and the two-stage fold of a duality-gap certificate's partial sums, shared by the single
// Chambolle-Pock solver (slp_cp.hip) and the two single ADMM solvers (slp_admm.hip, slp_admm_cg.hip): one text, so all three
// certificates add their terms in the order include/slp_hip_ext_cp_gap.h states.  A pass over `count` terms has S =
// cp_gap_slices(count) slices, one per lane group of its launch: term r belongs to slice r mod S, a slice adds its terms from 0.0 in increasing r -- whatever the format and the
// lanes per row.  The kernels are static: each translation unit that includes this header carries its own copy of the code.
#pragma once
#include "slp_cp_gap.h"
#include "slp_kernels.h"

namespace slp {

constexpr int kGapBlocks = 512;
inline i64 cp_gap_slices(i64 count) {
    i64 blocks = (count + kBlock - 1) / kBlock;
    blocks = blocks < 1 ? 1 : (blocks > kGapBlocks ? kGapBlocks : blocks);
    return blocks * kBlock;
}

// NaN-propagating maximum of one double per thread, valid in thread 0 (block_reduce<true> drops a NaN)
__device__ __forceinline__ double block_nan_max(double v, double *lds /* >= blockDim.x / kWave */) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = nan_max(v, __shfl_down(v, off, kWave));
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    if (lane == 0) lds[w] = v;
    __syncthreads();
    double r = v;
    if (threadIdx.x == 0) {
        r = lds[0];
        for (int i = 1; i < (int)(blockDim.x / kWave); ++i) r = nan_max(r, lds[i]);
    }
    __syncthreads();
    return r;
}

// The fold of the slice sums, two stages in a fixed order.  k_cp_gap_fold: workgroup q of a pass holds its slices 256 q .. 256 q + 255,
// one per lane, and adds them in the workgroup's fixed tree (a wavefront by halving, the four wavefronts in increasing order); the
// column pass's workgroups come first, the row pass's behind them.  bp[2 q], bp[2 q + 1]: the two quantities of workgroup q.
static __global__ __launch_bounds__(kBlock) void k_cp_gap_fold(i64 scols, const double *__restrict__ cp, i64 srows,
                                                               const double *__restrict__ rp, double *__restrict__ bp) {
    __shared__ double lds[kBlock / kWave];
    const i64 colblocks = scols / kBlock;
    const bool rows = (i64)blockIdx.x >= colblocks;   // uniform over the workgroup
    const i64 slice = (rows ? (i64)blockIdx.x - colblocks : (i64)blockIdx.x) * kBlock + threadIdx.x;
    const double q0 = rows ? rp[slice] : cp[slice], q1 = rows ? rp[srows + slice] : cp[scols + slice];
    const double r0 = block_reduce<false>(q0, lds);
    const double r1 = rows ? block_nan_max(q1, lds) : block_reduce<false>(q1, lds);
    if (threadIdx.x == 0) {
        bp[2 * (i64)blockIdx.x] = r0;
        bp[2 * (i64)blockIdx.x + 1] = r1;
    }
}

// k_cp_gap_final, one workgroup: lane l adds the sums of the workgroups l and l + 256 of a pass (at most 512) from 0.0, then the same tree.
// out[0] = c.x, out[1] = the bound's column terms, out[2] = y.b over this rank's rows, out[3] = their violation
static __global__ __launch_bounds__(kBlock) void k_cp_gap_final(i64 colblocks, i64 rowblocks, const double *__restrict__ bp,
                                                                double *__restrict__ out) {
    __shared__ double lds[kBlock / kWave];
    double cx = 0.0, terms = 0.0, yb = 0.0, viol = 0.0;
    for (i64 i = threadIdx.x; i < colblocks; i += kBlock) {
        cx += bp[2 * i];
        terms += bp[2 * i + 1];
    }
    for (i64 i = threadIdx.x; i < rowblocks; i += kBlock) {
        yb += bp[2 * (colblocks + i)];
        viol = nan_max(viol, bp[2 * (colblocks + i) + 1]);
    }
    const double r0 = block_reduce<false>(cx, lds), r1 = block_reduce<false>(terms, lds), r2 = block_reduce<false>(yb, lds);
    const double r3 = block_nan_max(viol, lds);
    if (threadIdx.x == 0) {
        out[0] = r0;
        out[1] = r1;
        out[2] = r2;
        out[3] = r3;
    }
}

}  // namespace slp
