// slp_dga_shared.h -- the arithmetic of dual gradient ascent that slp_dga.hip (one LP) and slp_dga_batch.hip (B LPs over one
// constraint matrix) both run: every chain of additions exists once, here, so instance k of a batch is bit for bit the single
// solve of its data.  The bodies below are whole kernels minus their addressing: the single solver's kernels call them on its
// vectors, the batched kernels on the segment of the instance blockIdx.y.  blockIdx.x / gridDim.x mean the same in both.
// slp_dga_many.hip (a list of LPs with matrices of their own, one workgroup of 1024 lanes per LP, whole iterations inside a launch)
// runs the same bodies: the gradient pass and the block's scalars take (part index, lane in block, wave-sum slots) in place of
// blockIdx.x / threadIdx.x / one LDS array, so that a 1024-lane workgroup computes them as four "virtual blocks" of four waves,
// and the vectors an earlier stage of the same launch wrote are read through LD (DgaLoadWorkgroup).
#pragma once
#include <algorithm>
#include <vector>

#include "slp_common.h"
#include "slp_kernels.h"
#include "slp_dga_draws.h"

namespace slp {

constexpr int kDgaFusedMax = 8192;      // padded breakpoints of the fused search: 12 B each = 96 KiB of the CU's 160 KiB
constexpr int kDgaFusedAuto = 2048;     // the fused search is the default up to here (measured cross-over between 1976 and 3816)
constexpr int kDgaFusedThreads = 1024;
constexpr int kDgaTile = 1024;          // elements per scan tile: 256 threads x 4
constexpr int kDgaParts = 256;          // workgroups (= partial results) of the gradient pass
constexpr unsigned long long kKeyMax = ~0ull;

enum { DGA_NEG_STEP = 1, DGA_EMPTY = 2, DGA_RAND_DRY = 4, DGA_NAN = 8, DGA_NO_CROSSING = 16 };

struct DgaCtl {
    double t;                      // the step of the block in flight
    double gb;                     // g . b
    double minratio;               // min over g < 0 of y / -g (inequality block)
    unsigned long long consumed;   // tie draws taken so far
    long long k;                   // the last bisection's index
    int active;                    // the block's predicate: any g < 0 / any g != 0
    int nb;                        // breakpoints of the search in flight (columns with d_j != 0)
    unsigned int flags;            // sticky, DGA_*
    int frozen;                    // batch and list: 1 = the start is dual infeasible (energy -inf), it stands still; batch only:
                                   // kDgaStopped = its stopping test has retired the instance (every kernel tests the field for truth)
};

constexpr int kDgaStopped = 2;

struct DgaLoadPlain {   // written by an earlier launch
    __device__ __forceinline__ double operator()(const double *p) const { return *p; }
    __device__ __forceinline__ int operator()(const int *p) const { return *p; }
};
struct DgaLoadWorkgroup {   // global memory written by other lanes of this workgroup before the last barrier (as CpLoadWorkgroup)
    __device__ __forceinline__ double operator()(const double *p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ int operator()(const int *p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};

// block_reduce over one "virtual block": the 256 lanes (4 waves) whose lane in block is tl = 0 .. 255 -- a wave_sum / wave_max per
// wave, then the four wave results in order; valid where tl == 0.  slots: 4 doubles of LDS of this virtual block.  Two barriers:
// every thread of the workgroup calls it.  With 256-lane workgroups and tl = threadIdx.x it is block_reduce.
template <bool IS_MAX>
__device__ __forceinline__ double dga_block_reduce(double v, int tl, double *slots) {
    v = IS_MAX ? wave_max(v) : wave_sum(v);
    if ((tl & (kWave - 1)) == 0) slots[tl / kWave] = v;
    __syncthreads();
    double r = IS_MAX ? -__builtin_inf() : 0.0;
    if (tl == 0) {
        r = slots[0];
#pragma unroll
        for (int i = 1; i < kBlock / kWave; ++i) {
            if (IS_MAX) r = (slots[i] > r) ? slots[i] : r;
            else r += slots[i];
        }
    }
    __syncthreads();
    return r;
}

// "any lane of the virtual block": valid in all its lanes.  Two barriers.
__device__ __forceinline__ int dga_block_or(int v, int tl, double *slots) {
    const int w = __any(v);
    if ((tl & (kWave - 1)) == 0) slots[tl / kWave] = w ? 1.0 : 0.0;
    __syncthreads();
    const int r = (slots[0] != 0.0) | (slots[1] != 0.0) | (slots[2] != 0.0) | (slots[3] != 0.0);
    __syncthreads();
    return r;
}

// order-preserving 64-bit image of a double; -0.0 and +0.0 share one key (numpy's sort takes them as equal)
__device__ __forceinline__ unsigned long long key_of(double a) {
    a = a + 0.0;
    const unsigned long long u = (unsigned long long)__double_as_longlong(a);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double wave_incl_scan(double v) {
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const double o = __shfl_up(v, off, kWave);
        if (lane >= off) v = o + v;
    }
    return v;
}

// Over every group of 4 waves (256 threads) of the workgroup: the exclusive prefix of `tot` among the group's threads and the
// group's total.  lds: one double per wave of the workgroup.  Contains barriers: every thread of the workgroup calls it.
__device__ __forceinline__ void group_excl_scan(double tot, double *lds, double &excl, double &total) {
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave, w0 = w & ~3;
    const double inc = wave_incl_scan(tot);
    double ex = __shfl_up(inc, 1, kWave);
    if (lane == 0) ex = 0.0;
    __syncthreads();
    if (lane == kWave - 1) lds[w] = inc;
    __syncthreads();
    double woff = 0.0, all = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (w0 + i < w) woff += lds[w0 + i];
        all += lds[w0 + i];
    }
    excl = woff + ex;
    total = all;
}

// the four elements of thread `tl` (0..255) of scan tile `tile`: forward min(d ub, d lb) at positions r, backward max(..) at
// positions nb - 1 - r, r = 1024 tile + 4 tl + e; 0.0 beyond the nb breakpoints
template <bool BACKWARD, class LD = DgaLoadPlain>
__device__ __forceinline__ void tile_values(int tile, int tl, int nb, const int *__restrict__ cols, const double *__restrict__ d,
                                            const double *__restrict__ lb, const double *__restrict__ ub, double v[4], LD ld = LD()) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = tile * kDgaTile + 4 * tl + e;
        double val = 0.0;
        if (r < nb) {
            const int j = cols[BACKWARD ? nb - 1 - r : r];
            const double dj = ld(d + j), u = dj * ub[j], l = dj * lb[j];
            val = BACKWARD ? ((u > l) ? u : l) : ((u < l) ? u : l);
        }
        v[e] = val;
    }
}

template <class LD = DgaLoadPlain>
__device__ __forceinline__ double alpha_at(int p, const int *cols, const double *cbar, const double *d, LD ld = LD()) {
    const int j = cols[p];
    return -ld(cbar + j) / ld(d + j);
}

// numpy.searchsorted(-deriv, 0) (side="left": the bisection of npy_binsearch), the tie rule and the step (:55-65, :168-173)
template <class Deriv, class LD = DgaLoadPlain>
__device__ __forceinline__ void finish_search(DgaCtl *ctl, int nb, Deriv deriv, const int *cols, const double *cbar,
                                              const double *d, const double *rnd, unsigned long long rnd_base,
                                              unsigned long long rnd_count, int ineq, LD ld = LD()) {
    if (nb == 0) {
        ctl->flags |= DGA_EMPTY;
        ctl->t = 0.0;
        return;
    }
    int lo = 0, hi = nb + 1;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (-deriv(mid) < 0.0) lo = mid + 1;
        else hi = mid;
    }
    const int k = lo;
    ctl->k = k;
    if (k > nb) {   // no sign change on the whole line (the reference's IndexError)
        ctl->flags |= DGA_NO_CROSSING;
        ctl->t = 0.0;
        return;
    }
    const int km1 = k == 0 ? nb - 1 : k - 1;
    double t;
    if (k < nb && deriv(k) == 0.0) {
        const unsigned long long at = ctl->consumed;
        double r = 0.5;
        if (at >= rnd_base && at - rnd_base < rnd_count) r = rnd[at - rnd_base];
        else ctl->flags |= DGA_RAND_DRY;
        ctl->consumed = at + 1;
        t = r * alpha_at(k, cols, cbar, d, ld) + (1.0 - r) * alpha_at(km1, cols, cbar, d, ld);
    } else {
        t = alpha_at(km1, cols, cbar, d, ld);
    }
    if (!(t >= 0.0)) ctl->flags |= DGA_NEG_STEP;
    if (t != t) ctl->flags |= DGA_NAN;
    if (ineq && ctl->minratio < t) t = ctl->minratio;
    ctl->t = t;
}

// ---- elementwise ---------------------------------------------------------------------------------------------------------------

// x_j = lb where c_bar > 0, ub where < 0, the midpoint where == 0 (:103-115)
__device__ __forceinline__ double dga_argmin_x(double cb, double l, double u) {
    double xv = 0.0;
    if (cb > 0.0) xv = l;
    else if (cb < 0.0) xv = u;
    else if (cb == 0.0) xv = 0.5 * (l + u);
    return xv;
}

// y_i + t g_i, inequality rows clamped at 0
__device__ __forceinline__ double dga_update_y(double yi, double t, double gi, int ineq) {
    double v = yi + t * gi;
    if (ineq && !(v > 0.0)) v = (v != v) ? v : 0.0;
    return v;
}

// ---- the gradient pass ---------------------------------------------------------------------------------------------------------

// The gradient of rows r0 .. r1 (0.0 elsewhere: the vector K^T multiplies), masked where y <= 0 on inequality rows (:159-161),
// and per part: g . b over its tiles of 256 rows (each a shuffle tree, the tiles in order), any g < 0 (inequalities) / any
// g != 0 (equalities), min y / -g over g < 0.  ax == NULL: g is given (slp_dga_line_search).
// Part `part` of `parts` covers tiles part * per .. (part + 1) * per, per = ceil(tiles / parts); a part without tiles gives
// (0.0, +inf, 0).  It is computed by one virtual block (tl: the lane in it, slots: its 4 doubles of LDS) in `steps` rounds of
// barriers, which every thread of the workgroup runs: the part's own tile count where a workgroup is one virtual block (the single
// and the batched solver: part = blockIdx.x, parts = gridDim.x, tl = threadIdx.x), `per` where four of them share a workgroup.
template <class LD = DgaLoadPlain>
__device__ __forceinline__ void dga_grad_body(i64 m, i64 r0, i64 r1, int ineq, const double *__restrict__ ax, const double *__restrict__ b,
                                              const double *__restrict__ y, double *__restrict__ g, double *__restrict__ part_gb,
                                              double *__restrict__ part_min, int *__restrict__ part_any, int part, int parts, int tl,
                                              i64 steps, double *slots, LD ld = LD()) {
    const i64 tiles = (m + kBlock - 1) / kBlock, per = (tiles + parts - 1) / parts;
    const i64 t0 = (i64)part * per, t1 = (t0 + per < tiles) ? t0 + per : tiles;
    double acc = 0.0, mn = __builtin_inf();
    int any = 0;
    for (i64 step = 0; step < steps; ++step) {
        const i64 t = t0 + step, i = t * kBlock + tl;
        double gi = 0.0, term = 0.0;
        if (t < t1 && i < m) {
            if (ax) {
                if (i >= r0 && i < r1) {
                    gi = ld(ax + i) - b[i];
                    if (ineq && ld(y + i) <= 0.0 && !(gi > 0.0)) gi = (gi != gi) ? gi : 0.0;
                }
                g[i] = gi;
            } else {
                gi = g[i];
            }
            term = gi * b[i];
            if (gi == 0.0) term = 0.0;   // (a zero of g is no stored entry of the sparse direction: b may be infinite there)
            if (ineq) {
                if (gi < 0.0) {
                    any = 1;
                    const double r = y ? ld(y + i) / -gi : __builtin_inf();
                    mn = (r < mn) ? r : mn;
                }
            } else if (gi != 0.0) {
                any = 1;
            }
        }
        const double s = dga_block_reduce<false>(term, tl, slots);
        if (tl == 0 && t < t1) acc += s;
    }
    mn = -dga_block_reduce<true>(-mn, tl, slots);
    any = dga_block_or(any, tl, slots);
    if (tl == 0) {
        part_gb[part] = acc;
        part_min[part] = mn;
        part_any[part] = any;
    }
}

// the tiles part `part` of `parts` holds of m rows: the `steps` of a workgroup that is one virtual block
__device__ __forceinline__ i64 dga_part_tiles(i64 m, int part, int parts) {
    const i64 tiles = (m + kBlock - 1) / kBlock, per = (tiles + parts - 1) / parts;
    const i64 t0 = (i64)part * per, t1 = (t0 + per < tiles) ? t0 + per : tiles;
    return t1 > t0 ? t1 - t0 : 0;
}

// the block's scalars from the partial results, reduced as one more 256-lane tile by a virtual block (tl, slots); `writer`: the
// virtual block whose lane 0 stores them (every virtual block of the workgroup runs the barriers)
template <class LD = DgaLoadPlain>
__device__ __forceinline__ void dga_begin_body(int parts, const double *__restrict__ part_gb, const double *__restrict__ part_min,
                                               const int *__restrict__ part_any, DgaCtl *__restrict__ ctl, int tl, double *slots,
                                               bool writer = true, LD ld = LD()) {
    const int i = tl;
    const double gb = dga_block_reduce<false>(i < parts ? ld(part_gb + i) : 0.0, tl, slots);
    const double mn = -dga_block_reduce<true>(i < parts ? -ld(part_min + i) : -__builtin_inf(), tl, slots);
    const int any = dga_block_or(i < parts ? ld(part_any + i) : 0, tl, slots);
    if (i == 0 && writer) {
        ctl->gb = gb;
        ctl->minratio = mn;
        ctl->active = any;
        ctl->nb = 0;
        ctl->t = 0.0;
    }
}

// ---- the search, general form --------------------------------------------------------------------------------------------------

// keys of the n columns (d_j == 0: the maximal key), cols[j] = j, ctl->nb += the breakpoints
__device__ __forceinline__ void dga_keys_body(int n, const double *__restrict__ d, const double *__restrict__ cbar,
                                              unsigned long long *__restrict__ keys, int *__restrict__ cols, DgaCtl *__restrict__ ctl) {
    int cnt = 0, bad = 0;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const double dj = d[j];
        unsigned long long key = kKeyMax;
        if (dj != 0.0) {
            const double a = -cbar[j] / dj;
            if (a != a) bad = 1;
            else { key = key_of(a); ++cnt; }
        }
        keys[j] = key;
        cols[j] = j;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && cnt) atomicAdd(&ctl->nb, cnt);
    if (bad) atomicOr(&ctl->flags, (unsigned int)DGA_NAN);
}

// tile sums of both scans: workgroup = tile blockIdx.x.  lds: kBlock / kWave doubles.
__device__ __forceinline__ void dga_tile_sums_body(const DgaCtl *__restrict__ ctl, const int *__restrict__ cols, const double *__restrict__ d,
                                                   const double *__restrict__ lb, const double *__restrict__ ub, double *__restrict__ tot_f,
                                                   double *__restrict__ tot_b, double *lds) {
    const int nb = ctl->nb, tile = blockIdx.x;
    if ((i64)tile * kDgaTile >= nb) return;
    double v[4], ex, total;
    tile_values<false>(tile, threadIdx.x, nb, cols, d, lb, ub, v);
    group_excl_scan(((v[0] + v[1]) + v[2]) + v[3], lds, ex, total);
    if (threadIdx.x == 0) tot_f[tile] = total;
    tile_values<true>(tile, threadIdx.x, nb, cols, d, lb, ub, v);
    group_excl_scan(((v[0] + v[1]) + v[2]) + v[3], lds, ex, total);
    if (threadIdx.x == 0) tot_b[tile] = total;
}

// Exclusive scan of `tiles` tile sums by the first 256 threads of the workgroup, in place: thread i sums its `per` consecutive
// tiles in order, the threads are scanned as in a tile, a tile's offset continues the chain from its thread's offset.
__device__ __forceinline__ void scan_tile_sums(int tiles, double *tot, double *lds) {
    const int per = (tiles + kBlock - 1) / kBlock, i0 = (int)threadIdx.x * per;
    const bool mine = threadIdx.x < kBlock;
    double s = 0.0;
    if (mine)
        for (int i = i0; i < i0 + per && i < tiles; ++i) s += tot[i];
    double ex, total;
    group_excl_scan(mine ? s : 0.0, lds, ex, total);
    if (mine) {
        double run = ex;
        for (int i = i0; i < i0 + per && i < tiles; ++i) {
            const double v = tot[i];
            tot[i] = run;
            run += v;
        }
    }
}

// F[p] = sum of min(..) over positions <= p, B[p] = sum of max(..) over positions >= p; workgroup = tile blockIdx.x
__device__ __forceinline__ void dga_scans_body(const DgaCtl *__restrict__ ctl, const int *__restrict__ cols, const double *__restrict__ d,
                                               const double *__restrict__ lb, const double *__restrict__ ub, const double *__restrict__ off_f,
                                               const double *__restrict__ off_b, double *__restrict__ F, double *__restrict__ B, double *lds) {
    const int nb = ctl->nb, tile = blockIdx.x;
    if ((i64)tile * kDgaTile >= nb) return;
    double v[4], ex, total;
    tile_values<false>(tile, threadIdx.x, nb, cols, d, lb, ub, v);
    group_excl_scan(((v[0] + v[1]) + v[2]) + v[3], lds, ex, total);
    double run = off_f[tile] + ex;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = tile * kDgaTile + 4 * (int)threadIdx.x + e;
        run += v[e];
        if (r < nb) F[r] = run;
    }
    tile_values<true>(tile, threadIdx.x, nb, cols, d, lb, ub, v);
    group_excl_scan(((v[0] + v[1]) + v[2]) + v[3], lds, ex, total);
    run = off_b[tile] + ex;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = tile * kDgaTile + 4 * (int)threadIdx.x + e;
        run += v[e];
        if (r < nb) B[nb - 1 - r] = run;
    }
}

// one thread: the bisection over derivatives[k] = -(g.b), [:-1] += backward sums, [1:] += forward sums (:47-49)
__device__ __forceinline__ void dga_search_body(DgaCtl *__restrict__ ctl, const int *__restrict__ cols, const double *__restrict__ cbar,
                                                const double *__restrict__ d, const double *__restrict__ F, const double *__restrict__ B,
                                                const double *__restrict__ rnd, unsigned long long rnd_base, unsigned long long rnd_count,
                                                int ineq) {
    const int nb = ctl->nb;
    const double ngb = -ctl->gb;
    auto deriv = [&](int k) {
        double v = ngb;
        if (k < nb) v = v + B[k];
        if (k > 0) v = v + F[k - 1];
        return v;
    };
    finish_search(ctl, nb, deriv, cols, cbar, d, rnd, rnd_base, rnd_count, ineq);
}

// ---- the search, fused form: one workgroup of kDgaFusedThreads, breakpoints in LDS ---------------------------------------------

inline size_t fused_lds_bytes(int npad) { return (size_t)npad * 12 + 40 * sizeof(double); }

// dga_lds: fused_lds_bytes(npad) bytes, 16-byte aligned:
// [npad] 8-byte slots (keys, then the derivative) | [npad] columns | 16 wave sums | 8 tile sums forward | 8 backward | scalars
template <class LD = DgaLoadPlain>
__device__ __forceinline__ void dga_fused_body(int n, int npad, const double *__restrict__ d, const double *__restrict__ cbar,
                                               const double *__restrict__ lb, const double *__restrict__ ub, DgaCtl *__restrict__ ctl,
                                               const double *__restrict__ rnd, unsigned long long rnd_base, unsigned long long rnd_count,
                                               int ineq, unsigned char *dga_lds, LD ld = LD()) {
    unsigned long long *slot = reinterpret_cast<unsigned long long *>(dga_lds);
    double *slotd = reinterpret_cast<double *>(dga_lds);
    int *cols = reinterpret_cast<int *>(dga_lds + (size_t)npad * 8);
    double *lds = reinterpret_cast<double *>(dga_lds + (size_t)npad * 12);
    double *tot_f = lds + 16, *tot_b = lds + 24, *last = lds + 32;
    int *cnt = reinterpret_cast<int *>(lds + 33);
    const int tid = threadIdx.x;
    if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
    __syncthreads();
    int mine = 0, bad = 0;
    for (int j = tid; j < npad; j += kDgaFusedThreads) {
        unsigned long long key = kKeyMax;
        int col = 0x7fffffff;
        if (j < n) {
            col = j;
            const double dj = ld(d + j);
            if (dj != 0.0) {
                const double a = -ld(cbar + j) / dj;
                if (a != a) bad = 1;
                else { key = key_of(a); ++mine; }
            }
        }
        slot[j] = key;
        cols[j] = col;
    }
    if (mine) atomicAdd(&cnt[0], mine);
    if (bad) atomicOr(&cnt[1], 1);
    __syncthreads();
    // bitonic sort, ascending on (key, column): the order of a stable sort by key
    for (int size = 2; size <= npad; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (npad >> 1); i += kDgaFusedThreads) {
                const int a = 2 * i - (i & (stride - 1)), b = a + stride;
                const bool up = (a & size) == 0;
                const unsigned long long ka = slot[a], kb = slot[b];
                const int ca = cols[a], cb = cols[b];
                const bool gt = ka > kb || (ka == kb && ca > cb);
                if (gt == up) {
                    slot[a] = kb; slot[b] = ka;
                    cols[a] = cb; cols[b] = ca;
                }
            }
            __syncthreads();
        }
    }
    const int nb = cnt[0];
    const int tiles = (nb + kDgaTile - 1) / kDgaTile, group = tid >> 8, tl = tid & 255;
    const double ngb = -ctl->gb;
    double v[4], ex, total;
    // tile sums (4 tiles per pass: one per group of 4 waves), their scan, then the final passes
    for (int t0 = 0; t0 < tiles; t0 += 4) {
        const int tile = t0 + group;
        tile_values<false>(tile, tl, nb, cols, d, lb, ub, v, ld);
        group_excl_scan(((v[0] + v[1]) + v[2]) + v[3], lds, ex, total);
        if (tl == 0 && tile < tiles) tot_f[tile] = total;
        tile_values<true>(tile, tl, nb, cols, d, lb, ub, v, ld);
        group_excl_scan(((v[0] + v[1]) + v[2]) + v[3], lds, ex, total);
        if (tl == 0 && tile < tiles) tot_b[tile] = total;
    }
    __syncthreads();
    scan_tile_sums(tiles, tot_f, lds);
    scan_tile_sums(tiles, tot_b, lds);
    __syncthreads();
    // backward: slot[p] = -(g.b) + B[p]
    for (int t0 = 0; t0 < tiles; t0 += 4) {
        const int tile = t0 + group;
        tile_values<true>(tile, tl, nb, cols, d, lb, ub, v, ld);
        group_excl_scan(((v[0] + v[1]) + v[2]) + v[3], lds, ex, total);
        double run = (tile < tiles ? tot_b[tile] : 0.0) + ex;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = tile * kDgaTile + 4 * tl + e;
            run += v[e];
            if (r < nb) slotd[nb - 1 - r] = ngb + run;
        }
    }
    __syncthreads();
    // forward: derivative[p + 1] += F[p]; the last one has no backward part
    for (int t0 = 0; t0 < tiles; t0 += 4) {
        const int tile = t0 + group;
        tile_values<false>(tile, tl, nb, cols, d, lb, ub, v, ld);
        group_excl_scan(((v[0] + v[1]) + v[2]) + v[3], lds, ex, total);
        double run = (tile < tiles ? tot_f[tile] : 0.0) + ex;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = tile * kDgaTile + 4 * tl + e;
            run += v[e];
            if (r + 1 < nb) slotd[r + 1] = slotd[r + 1] + run;
            else if (r + 1 == nb) last[0] = ngb + run;
        }
    }
    __syncthreads();
    if (tid == 0) {
        ctl->nb = nb;
        if (cnt[1]) ctl->flags |= DGA_NAN;
        auto deriv = [&](int k) { return k < nb ? slotd[k] : last[0]; };
        finish_search(ctl, nb, deriv, cols, cbar, d, rnd, rnd_base, rnd_count, ineq, ld);
    }
}

// ---- report ------------------------------------------------------------------------------------------------------------------

// per workgroup: sum over c_bar != 0 of min(c_bar ub, c_bar lb) (:121-123).  red: kBlock / kWave doubles.
__device__ __forceinline__ void dga_energy_x_body(i64 n, const double *__restrict__ cbar, const double *__restrict__ lb,
                                                  const double *__restrict__ ub, double *__restrict__ part, double *red) {
    double acc = 0.0;
    for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (i64)gridDim.x * blockDim.x) {
        const double cb = cbar[j];
        if (cb != 0.0) {
            const double u = cb * ub[j], l = cb * lb[j];
            acc += (u < l) ? u : l;
        }
    }
    acc = block_reduce<false>(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// per workgroup: y . b and, with VIOL, the largest violation (a_i x - b_i on inequality rows, |a_i x - b_i| on equality rows) and
// their sum; without VIOL (the bound alone: the batch's stopping test) `ax` is not looked at and only the first slot is written
template <bool VIOL = true>
__device__ __forceinline__ void dga_energy_y_body(i64 m, i64 m_eq, const double *__restrict__ y, const double *__restrict__ b,
                                                  const double *__restrict__ ax, double *__restrict__ part, double *red) {
    double yb = 0.0, mx = -__builtin_inf(), sum = 0.0;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (i64)gridDim.x * blockDim.x) {
        if (y[i] != 0.0) yb += y[i] * b[i];
        if (VIOL) {
            double r = ax[i] - b[i];
            if (i < m_eq) r = fabs(r);
            mx = (r > mx) ? r : mx;
            if (r > 0.0) sum += r;
        }
    }
    yb = block_reduce<false>(yb, red);
    if (VIOL) {
        mx = block_reduce<true>(mx, red);
        sum = block_reduce<false>(sum, red);
    }
    if (threadIdx.x == 0) {
        part[3 * blockIdx.x] = yb;
        if (VIOL) {
            part[3 * blockIdx.x + 1] = mx;
            part[3 * blockIdx.x + 2] = sum;
        }
    }
}

// the dual energy from the kDgaParts partial results of both passes (h[0 .. parts): energy_x, h[parts + 3 i]: the y . b of
// energy_y), each summed in order: the report's on the host and, for the batch's stopping test, one lane's on the device
__host__ __device__ inline double dga_bound_finish(const double *h) {
    double e = 0.0, yb = 0.0;
    for (int i = 0; i < kDgaParts; ++i) {
        e += h[(size_t)i];
        yb += h[(size_t)(kDgaParts + 3 * i)];
    }
    return e - yb;
}

// host: the kDgaParts partial results of both passes (h[0 .. parts): energy_x, h[parts .. 4 parts): energy_y) in order
inline void dga_report_finish(const double *h, bool has_rows, double out[3]) {
    double mx = -__builtin_inf(), sum = 0.0;
    for (int i = 0; i < kDgaParts; ++i) {
        mx = std::max(mx, h[(size_t)(kDgaParts + 3 * i + 1)]);
        sum += h[(size_t)(kDgaParts + 3 * i + 2)];
    }
    out[0] = dga_bound_finish(h);
    out[1] = has_rows ? mx : 0.0;
    out[2] = sum;
}

// ---- host: stage timing ----------------------------------------------------------------------------------------------------------

enum { ST_PRODUCTS = 0, ST_SORT = 1, ST_SCANS = 2, ST_REST = 3, ST_FUSED = 4, ST_COUNT = 5 };

// HIP events at the stage boundaries of the iterations while switched on; read after the timed region
struct StageTimer {
    bool on = false;
    std::vector<hipEvent_t> ev;
    std::vector<int> tag;   // the stage that ended at event k (-1: the opening event of an iteration)
    size_t used = 0;
    ~StageTimer() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    void set(int enable) {
        on = enable != 0;
        if (on) used = 0;
    }
    void mark(int stage) {
        if (!on || used >= (1u << 20)) return;
        if (ev.size() <= used) {
            hipEvent_t e = nullptr;
            SLP_HIP(hipEventCreate(&e));
            ev.push_back(e);
            tag.push_back(0);
        }
        tag[used] = stage;
        SLP_HIP(hipEventRecord(ev[used], ctx().stream));
        ++used;
    }
    // milliseconds per stage since the timer was switched on
    void read(double out[ST_COUNT]) {
        for (int i = 0; i < ST_COUNT; ++i) out[i] = 0.0;
        if (used) SLP_HIP(hipEventSynchronize(ev[used - 1]));
        for (size_t k = 1; k < used; ++k) {
            if (tag[k] < 0) continue;
            float ms = 0.f;
            SLP_HIP(hipEventElapsedTime(&ms, ev[k - 1], ev[k]));
            out[tag[k]] += (double)ms;
        }
    }
};

// ---- what the batch and the list handles answer alike, from the controls `h` just read back and the window of draws --------------

// (flags, tie draws taken) per reader, then the draws left behind the furthest reader and the iterations done
inline void dga_status_out(const std::vector<DgaCtl> &h, const DgaDrawWindow &w, i64 iters, int64_t *out) {
    const size_t count = h.size();
    const unsigned int dry = w.dry ? (unsigned int)DGA_RAND_DRY : 0u;
    for (size_t k = 0; k < count; ++k) {
        out[2 * k] = (int64_t)(h[k].flags | dry);
        out[2 * k + 1] = (int64_t)h[k].consumed;
    }
    out[2 * count] = w.left();
    out[2 * count + 1] = iters;
}

inline void dga_frozen_out(const std::vector<DgaCtl> &h, int32_t *out) {
    for (size_t k = 0; k < h.size(); ++k) out[k] = h[k].frozen;
}

// what push_random does once the controls are read: `offset(k)` is where reader k's positions begin in the stream, `moves(k)`
// whether it still takes draws (dga_passed_by_all: the draws every moving reader has passed are dropped from the front)
template <class Offset, class Moves>
inline void dga_push_draws(const std::vector<DgaCtl> &h, Offset offset, Moves moves, DgaDrawWindow &w, DevBuf<double> &rnd,
                           const double *draws, int64_t count, DgaOverrun mode) {
    const uint64_t passed = dga_passed_by_all(h.size(), moves, [&](size_t k) { return (uint64_t)(offset(k) + h[k].consumed); });
    w.push(draws, count, passed, mode);
    if (w.size()) rnd.upload(w.data(), (size_t)w.size());
}

// the same with the readers of the batch: every instance that is not frozen moves
template <class Offset>
inline void dga_push_draws(const std::vector<DgaCtl> &h, Offset offset, DgaDrawWindow &w, DevBuf<double> &rnd, const double *draws,
                           int64_t count, DgaOverrun mode) {
    dga_push_draws(h, offset, [&](size_t k) { return !h[k].frozen; }, w, rnd, draws, count, mode);
}

}  // namespace slp
