// slp_dga.hip -- dual gradient ascent with the exact dual line search on the device (reference DualGradientAscent.py:36-245).
//
// One iteration (dga_iteration): c_bar = (c + A_e^T y_e) + A_i^T y_i and the dual argmin x (get_optim_x, :103-115), K x once,
// then for the inequality rows and for the equality rows (with the SAME c_bar and x, :145-209): the gradient g with its mask,
// d = K^T g, and the line search over the breakpoints alpha_j = -c_bar_j / d_j (exact_dual_line_search, :36-65): sort, a
// forward sum of min(d ub, d lb), a backward sum of max(d ub, d lb), the bisection of numpy.searchsorted on their derivative
// and the tie rule.  The products are the library's (matrix_spmv in SLP_ORDER_SEQUENTIAL: scipy's chains on every copy);
// the rows of the other kind are masked to 0.0, which leaves a running sum as it is.
//
// Nothing is read back inside slp_dga_iterate: the "skip this block" predicates, the step, the count of tie draws and the
// sticky status flags live in a DgaCtl in device memory.
//
// Two forms of the search, the same arithmetic (so the same bits) in both:
//   general -- keys of all n columns (d_j == 0: the maximal key, so n is never read back), rocprim::radix_sort_pairs (stable:
//              equal alpha stay in column order), tile sums / one-workgroup scan of the tile sums / final pass, bisection;
//   fused   -- at most kDgaFusedMax = 8192 variables, the default up to kDgaFusedAuto = 2048 (beyond, its 91 barrier-separated sort
//              stages cost more than the general form's launches: profiles/dga_small_paths.json): ONE workgroup of 1024 threads, 12 bytes of LDS per padded breakpoint (8-byte key +
//              4-byte column, 96 KiB at 8192): a bitonic sort on (key, column), then the backward sums overwrite the key slots
//              and the forward pass adds its sums in place, so the slots end as the derivative the bisection reads.
// A scan is: 4 consecutive elements per thread in order, Hillis-Steele over the 64 lanes, the 4 waves of a 1024-element tile in
// order, tile sums scanned the same way by one workgroup; an element's value continues the chain from its thread's offset.
// The device functions that fix this arithmetic (and the kernel bodies built from them) are in slp_dga_shared.h, shared with the
// batched solver (slp_dga_batch.hip): the kernels below call them on this solver's vectors.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "slp_common.h"
#include "slp_kernels.h"
#include "slp_dga_shared.h"

using namespace slp;

namespace {

// ---- elementwise passes ------------------------------------------------------------------------------------------------------

__global__ void k_dga_mask(i64 m, i64 lo, i64 hi, const double *__restrict__ y, double *__restrict__ out) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (i64)gridDim.x * blockDim.x)
        out[i] = (i >= lo && i < hi) ? y[i] : 0.0;
}

// c_bar = (c + s_eq) + s_ineq, x = lb where c_bar > 0, ub where < 0, the midpoint where == 0 (:103-115)
__global__ void k_dga_argmin(i64 n, const double *__restrict__ c, const double *__restrict__ se, const double *__restrict__ si,
                             const double *__restrict__ lb, const double *__restrict__ ub, double *__restrict__ cbar,
                             double *__restrict__ x) {
    for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (i64)gridDim.x * blockDim.x) {
        double cb = c[j];
        if (se) cb = cb + se[j];
        if (si) cb = cb + si[j];
        cbar[j] = cb;
        x[j] = dga_argmin_x(cb, lb[j], ub[j]);
    }
}

// the gradient pass (dga_grad_body): kDgaParts workgroups
__global__ void k_dga_grad(i64 m, i64 r0, i64 r1, int ineq, const double *__restrict__ ax, const double *__restrict__ b,
                           const double *__restrict__ y, double *__restrict__ g, double *__restrict__ part_gb,
                           double *__restrict__ part_min, int *__restrict__ part_any) {
    __shared__ double red[kBlock / kWave];
    dga_grad_body(m, r0, r1, ineq, ax, b, y, g, part_gb, part_min, part_any, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x,
                  dga_part_tiles(m, (int)blockIdx.x, (int)gridDim.x), red);
}

// one workgroup: the block's scalars from the partial results
__global__ void k_dga_begin(int parts, const double *__restrict__ part_gb, const double *__restrict__ part_min,
                            const int *__restrict__ part_any, DgaCtl *__restrict__ ctl) {
    __shared__ double red[kBlock / kWave];
    dga_begin_body(parts, part_gb, part_min, part_any, ctl, (int)threadIdx.x, red);
}

__global__ void k_dga_update(i64 r0, i64 r1, int ineq, const DgaCtl *__restrict__ ctl, const double *__restrict__ g,
                             double *__restrict__ y) {
    if (!ctl->active) return;
    const double t = ctl->t;
    for (i64 i = r0 + (i64)blockIdx.x * blockDim.x + threadIdx.x; i < r1; i += (i64)gridDim.x * blockDim.x)
        y[i] = dga_update_y(y[i], t, g[i], ineq);
}

// ---- the search, general form ------------------------------------------------------------------------------------------------

__global__ void k_dga_keys(int n, const double *__restrict__ d, const double *__restrict__ cbar, unsigned long long *__restrict__ keys,
                           int *__restrict__ cols, DgaCtl *__restrict__ ctl) {
    if (!ctl->active) return;
    dga_keys_body(n, d, cbar, keys, cols, ctl);
}

// tile sums of both scans: workgroup = tile
__global__ void k_dga_tile_sums(const DgaCtl *__restrict__ ctl, const int *__restrict__ cols, const double *__restrict__ d,
                                const double *__restrict__ lb, const double *__restrict__ ub, double *__restrict__ tot_f,
                                double *__restrict__ tot_b) {
    __shared__ double lds[kBlock / kWave];
    if (!ctl->active) return;
    dga_tile_sums_body(ctl, cols, d, lb, ub, tot_f, tot_b, lds);
}

__global__ void k_dga_tile_offsets(const DgaCtl *__restrict__ ctl, double *__restrict__ tot_f, double *__restrict__ tot_b) {
    __shared__ double lds[kBlock / kWave];
    if (!ctl->active) return;
    const int tiles = (ctl->nb + kDgaTile - 1) / kDgaTile;
    scan_tile_sums(tiles, tot_f, lds);
    scan_tile_sums(tiles, tot_b, lds);
}

// F[p] = sum of min(..) over positions <= p, B[p] = sum of max(..) over positions >= p
__global__ void k_dga_scans(const DgaCtl *__restrict__ ctl, const int *__restrict__ cols, const double *__restrict__ d,
                            const double *__restrict__ lb, const double *__restrict__ ub, const double *__restrict__ off_f,
                            const double *__restrict__ off_b, double *__restrict__ F, double *__restrict__ B) {
    __shared__ double lds[kBlock / kWave];
    if (!ctl->active) return;
    dga_scans_body(ctl, cols, d, lb, ub, off_f, off_b, F, B, lds);
}

__global__ void k_dga_search(DgaCtl *__restrict__ ctl, const int *__restrict__ cols, const double *__restrict__ cbar,
                             const double *__restrict__ d, const double *__restrict__ F, const double *__restrict__ B,
                             const double *__restrict__ rnd, unsigned long long rnd_base, unsigned long long rnd_count, int ineq) {
    if (!ctl->active || threadIdx.x != 0 || blockIdx.x != 0) return;
    dga_search_body(ctl, cols, cbar, d, F, B, rnd, rnd_base, rnd_count, ineq);
}

// ---- the search, fused form: one workgroup, breakpoints in LDS -----------------------------------------------------------------

__global__ void __launch_bounds__(kDgaFusedThreads)
k_dga_fused(int n, int npad, const double *__restrict__ d, const double *__restrict__ cbar, const double *__restrict__ lb,
            const double *__restrict__ ub, DgaCtl *__restrict__ ctl, const double *__restrict__ rnd, unsigned long long rnd_base,
            unsigned long long rnd_count, int ineq) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dga_lds[];
    if (!ctl->active) return;
    dga_fused_body(n, npad, d, cbar, lb, ub, ctl, rnd, rnd_base, rnd_count, ineq, dga_lds);
}

// ---- report ------------------------------------------------------------------------------------------------------------------

__global__ void k_dga_energy_x(i64 n, const double *__restrict__ cbar, const double *__restrict__ lb, const double *__restrict__ ub,
                               double *__restrict__ part) {
    __shared__ double red[kBlock / kWave];
    dga_energy_x_body(n, cbar, lb, ub, part, red);
}

__global__ void k_dga_energy_y(i64 m, i64 m_eq, const double *__restrict__ y, const double *__restrict__ b, const double *__restrict__ ax,
                               double *__restrict__ part) {
    __shared__ double red[kBlock / kWave];
    dga_energy_y_body(m, m_eq, y, b, ax, part, red);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

// what one line search works in: n columns
struct DgaSearch {
    int n = 0, npad = 0, tiles = 0;
    bool fused = false;
    DevBuf<DgaCtl> ctl;
    DevBuf<double> d, F, B, tot_f, tot_b, part_gb, part_min;
    DevBuf<int> part_any, cols, cols_sorted;
    DevBuf<unsigned long long> keys, keys_sorted;
    DevBuf<unsigned char> sort_tmp;
    size_t sort_bytes = 0;
    DevBuf<double> rnd;
    DgaDrawWindow draws;                   // the host's view of rnd (slp_dga_draws.h)
    StageTimer timer;
};

void search_setup(DgaSearch &w, i64 n, int path) {
    SLP_REQUIRE(n > 0 && n < ((i64)1 << 31) - kDgaTile, "dual gradient ascent: the number of variables must be in 1 .. 2^31 - 1025");
    w.n = (int)n;
    int npad = 64;
    while (npad < n && npad < (1 << 30)) npad <<= 1;
    w.npad = npad;
    SLP_REQUIRE(path >= 0 && path <= 2, "dual gradient ascent: path must be 0 (auto), 1 (fused) or 2 (general)");
    SLP_REQUIRE(path != 1 || n <= kDgaFusedMax, "dual gradient ascent: the fused search holds at most 8192 variables");
    w.fused = path == 1 || (path == 0 && n <= kDgaFusedAuto);
    w.tiles = (int)((n + kDgaTile - 1) / kDgaTile);
    w.ctl.alloc(1);
    w.ctl.zero();
    w.d.alloc((size_t)n);
    w.part_gb.alloc(kDgaParts); w.part_min.alloc(kDgaParts); w.part_any.alloc(kDgaParts);
    w.cols.alloc((size_t)n);   // (the fused form keeps its columns in LDS; alpha_at of the general form reads cols_sorted)
    if (w.fused) {
        SLP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dga_fused), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)fused_lds_bytes(kDgaFusedMax)));
        return;
    }
    w.F.alloc((size_t)n); w.B.alloc((size_t)n);
    w.tot_f.alloc((size_t)w.tiles); w.tot_b.alloc((size_t)w.tiles);
    w.cols_sorted.alloc((size_t)n); w.keys.alloc((size_t)n); w.keys_sorted.alloc((size_t)n);
    SLP_HIP(rocprim::radix_sort_pairs(nullptr, w.sort_bytes, w.keys.p, w.keys_sorted.p, w.cols.p, w.cols_sorted.p, (size_t)n, 0u, 64u,
                                      ctx().stream));
    w.sort_tmp.alloc(w.sort_bytes ? w.sort_bytes : 1);
}

// Appends draws to the device buffer (the draws already taken are dropped from its front).  Synchronises.
void search_push_random(DgaSearch &w, const double *r, i64 count) {
    DgaCtl h;
    w.ctl.download(&h, 1);
    w.draws.push(r, count, h.consumed, kJump);
    if (w.draws.size()) w.rnd.upload(w.draws.data(), (size_t)w.draws.size());
}

// g (m values, already on the device), its partial results -> the block's scalars -> d = K^T g -> the step in ctl->t
void search_run(DgaSearch &w, slp_matrix *k, i64 m, const double *g, const double *cbar, const double *lb, const double *ub, int ineq) {
    hipStream_t st = ctx().stream;
    hipLaunchKernelGGL(k_dga_begin, dim3(1), dim3(kBlock), 0, st, kDgaParts, w.part_gb.p, w.part_min.p, w.part_any.p, w.ctl.p);
    w.timer.mark(ST_REST);
    if (m > 0) matrix_spmv(k, true, g, w.d.p, SLP_ORDER_SEQUENTIAL);
    else w.d.zero();
    w.timer.mark(ST_PRODUCTS);
    const unsigned long long rb = w.draws.base, rc = w.draws.size();
    if (w.fused) {
        int npad = w.npad;
        hipLaunchKernelGGL(k_dga_fused, dim3(1), dim3(kDgaFusedThreads), fused_lds_bytes(npad), st, w.n, npad, w.d.p, cbar, lb, ub, w.ctl.p,
                           w.rnd.p, rb, rc, ineq);
        SLP_HIP(hipGetLastError());
        w.timer.mark(ST_FUSED);
        return;
    }
    hipLaunchKernelGGL(k_dga_keys, dim3(grid_for(w.n, kBlock)), dim3(kBlock), 0, st, w.n, w.d.p, cbar, w.keys.p, w.cols.p, w.ctl.p);
    SLP_HIP(hipGetLastError());
    w.timer.mark(ST_REST);
    size_t bytes = w.sort_bytes;
    SLP_HIP(rocprim::radix_sort_pairs(w.sort_tmp.p, bytes, w.keys.p, w.keys_sorted.p, w.cols.p, w.cols_sorted.p, (size_t)w.n, 0u, 64u, st));
    w.timer.mark(ST_SORT);
    hipLaunchKernelGGL(k_dga_tile_sums, dim3(w.tiles), dim3(kBlock), 0, st, w.ctl.p, w.cols_sorted.p, w.d.p, lb, ub, w.tot_f.p, w.tot_b.p);
    hipLaunchKernelGGL(k_dga_tile_offsets, dim3(1), dim3(kBlock), 0, st, w.ctl.p, w.tot_f.p, w.tot_b.p);
    hipLaunchKernelGGL(k_dga_scans, dim3(w.tiles), dim3(kBlock), 0, st, w.ctl.p, w.cols_sorted.p, w.d.p, lb, ub, w.tot_f.p, w.tot_b.p, w.F.p,
                       w.B.p);
    SLP_HIP(hipGetLastError());
    w.timer.mark(ST_SCANS);
    hipLaunchKernelGGL(k_dga_search, dim3(1), dim3(kWave), 0, st, w.ctl.p, w.cols_sorted.p, cbar, w.d.p, w.F.p, w.B.p, w.rnd.p, rb, rc,
                       ineq);
    SLP_HIP(hipGetLastError());
    w.timer.mark(ST_REST);
}

}  // namespace

struct slp_dga {
    slp_matrix *k = nullptr;
    i64 n = 0, m = 0, m_eq = 0;
    DevBuf<double> b, c, lb, ub, y, x, cbar, se, si, ymask, ax, g, rcbar, rx, rax, rpart;
    DgaSearch w;
    i64 iters = 0;
};

namespace {

// c_bar and x of the multipliers y into (cbar, x): the two partial column sums apart, as the reference adds them (:104-108)
void dga_argmin(slp_dga *s, double *cbar, double *x) {
    hipStream_t st = ctx().stream;
    const i64 n = s->n, m = s->m, me = s->m_eq;
    const double *se = nullptr, *si = nullptr;
    if (me > 0 && me < m) {
        hipLaunchKernelGGL(k_dga_mask, dim3(grid_for(m, kBlock)), dim3(kBlock), 0, st, m, (i64)0, me, s->y.p, s->ymask.p);
        matrix_spmv(s->k, true, s->ymask.p, s->se.p, SLP_ORDER_SEQUENTIAL);
        hipLaunchKernelGGL(k_dga_mask, dim3(grid_for(m, kBlock)), dim3(kBlock), 0, st, m, me, m, s->y.p, s->ymask.p);
        matrix_spmv(s->k, true, s->ymask.p, s->si.p, SLP_ORDER_SEQUENTIAL);
        se = s->se.p;
        si = s->si.p;
    } else if (m > 0) {
        matrix_spmv(s->k, true, s->y.p, s->se.p, SLP_ORDER_SEQUENTIAL);
        (me > 0 ? se : si) = s->se.p;
    }
    s->w.timer.mark(ST_PRODUCTS);
    hipLaunchKernelGGL(k_dga_argmin, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, st, n, s->c.p, se, si, s->lb.p, s->ub.p, cbar, x);
    SLP_HIP(hipGetLastError());
}

void dga_block(slp_dga *s, i64 r0, i64 r1, int ineq) {
    hipStream_t st = ctx().stream;
    hipLaunchKernelGGL(k_dga_grad, dim3(kDgaParts), dim3(kBlock), 0, st, s->m, r0, r1, ineq, s->ax.p, s->b.p, s->y.p, s->g.p, s->w.part_gb.p,
                       s->w.part_min.p, s->w.part_any.p);
    search_run(s->w, s->k, s->m, s->g.p, s->cbar.p, s->lb.p, s->ub.p, ineq);
    hipLaunchKernelGGL(k_dga_update, dim3(grid_for(r1 - r0, kBlock)), dim3(kBlock), 0, st, r0, r1, ineq, s->w.ctl.p, s->g.p, s->y.p);
    SLP_HIP(hipGetLastError());
    s->w.timer.mark(ST_REST);
}

void dga_iteration(slp_dga *s) {
    s->w.timer.mark(-1);
    dga_argmin(s, s->cbar.p, s->x.p);
    s->w.timer.mark(ST_REST);
    if (s->m > 0) matrix_spmv(s->k, false, s->x.p, s->ax.p, SLP_ORDER_SEQUENTIAL);
    s->w.timer.mark(ST_PRODUCTS);
    if (s->m > s->m_eq) dga_block(s, s->m_eq, s->m, 1);
    if (s->m_eq > 0) dga_block(s, 0, s->m_eq, 0);
}

unsigned int dga_read_ctl(slp_dga *s, DgaCtl *out) {
    DgaCtl h;
    s->w.ctl.download(&h, 1);
    s->w.draws.observe(h.consumed);
    if (out) *out = h;
    return h.flags | (s->w.draws.dry ? (unsigned int)DGA_RAND_DRY : 0u);
}

}  // namespace

extern "C" {

slp_dga *slp_dga_create_on(slp_matrix *a, int64_t m_eq, const double *b, const double *c, const double *lb, const double *ub,
                           const double *y0) {
    SLP_API_PTR({
        SLP_REQUIRE(a && c && lb && ub, "slp_dga_create_on: NULL argument");
        const i64 m = a->a.nrow, n = a->a.ncol;
        SLP_REQUIRE(m_eq >= 0 && m_eq <= m, "slp_dga_create_on: m_eq out of range");
        SLP_REQUIRE(m == 0 || (b && y0), "slp_dga_create_on: NULL argument");
        const bool csrless = !a->chunks.empty() || a->csr_released;
        if (csrless)
            SLP_REQUIRE(fast_format(a, false) && fast_format(a, true),
                        "slp_dga_create_on: the CSR entries of this matrix are gone and it has no strip copies in both orientations");
        auto *s = new slp_dga();
        try {
            int path = 0;
            if (const char *e = getenv("SLP_DGA_PATH")) path = !strcmp(e, "fused") ? 1 : (!strcmp(e, "general") ? 2 : 0);
            s->k = a; s->n = n; s->m = m; s->m_eq = m_eq;
            search_setup(s->w, n, path);
            if (!csrless) {   // formats are settled here, not inside an iteration
                ensure_transposed(a);
                fast_format(a, false);
                if (!fast_format(a, true)) build_transpose(a);
            }
            const size_t sn = (size_t)n, sm = (size_t)m;
            s->c.upload(c, sn); s->lb.upload(lb, sn); s->ub.upload(ub, sn);
            s->b.alloc(sm); s->y.alloc(sm);
            if (m) { s->b.upload(b, sm); s->y.upload(y0, sm); }
            s->x.alloc(sn); s->cbar.alloc(sn); s->se.alloc(sn); s->si.alloc(sn);
            s->ymask.alloc(sm); s->ax.alloc(sm); s->g.alloc(sm);
            dga_argmin(s, s->cbar.p, s->x.p);   // the x of y0: what a dual-infeasible start returns (:136-139)
            SLP_HIP(hipStreamSynchronize(ctx().stream));
        } catch (...) {
            delete s;
            throw;
        }
        ++a->borrowers;
        return s;
    })
}

void slp_dga_destroy(slp_dga *s) {
    if (!s) return;
    --s->k->borrowers;
    delete s;
}

int slp_dga_set_path(slp_dga *s, int path) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_dga_set_path: NULL handle");
        DgaCtl h;
        s->w.ctl.download(&h, 1);
        search_setup(s->w, s->n, path);
        SLP_HIP(hipMemcpyAsync(s->w.ctl.p, &h, sizeof(h), hipMemcpyHostToDevice, ctx().stream));
        SLP_HIP(hipStreamSynchronize(ctx().stream));
    })
}

int slp_dga_path(const slp_dga *s) { return s ? (s->w.fused ? 1 : 2) : -1; }

int slp_dga_iterate(slp_dga *s, int64_t k) {
    SLP_API_INT({
        SLP_REQUIRE(s && k >= 0, "slp_dga_iterate: bad arguments");
        for (i64 it = 0; it < k && s->w.draws.reserve(1); ++it) {   // at most two tie draws per iteration
            dga_iteration(s);
            ++s->iters;
        }
    })
}

int64_t slp_dga_iterations(const slp_dga *s) { return s ? s->iters : -1; }

int slp_dga_push_random(slp_dga *s, const double *draws, int64_t count) {
    SLP_API_INT({
        SLP_REQUIRE(s && count >= 0 && (draws || count == 0), "slp_dga_push_random: bad arguments");
        search_push_random(s->w, draws, count);
        dga_read_ctl(s, nullptr);
    })
}

int slp_dga_status(slp_dga *s, int64_t out[4]) {
    SLP_API_INT({
        SLP_REQUIRE(s && out, "slp_dga_status: NULL argument");
        DgaCtl h;
        out[0] = (int64_t)dga_read_ctl(s, &h);
        out[1] = (int64_t)h.consumed;
        out[2] = s->w.draws.left();
        out[3] = s->iters;
    })
}

int slp_dga_get_x(slp_dga *s, double *x) { SLP_API_INT({ SLP_REQUIRE(s && x, "NULL argument"); s->x.download(x, (size_t)s->n); }) }

int slp_dga_get_y(slp_dga *s, double *y) { SLP_API_INT({ SLP_REQUIRE(s && y, "NULL argument"); s->y.download(y, (size_t)s->m); }) }

int slp_dga_report(slp_dga *s, double out[3]) {
    SLP_API_INT({
        SLP_REQUIRE(s && out, "slp_dga_report: NULL argument");
        hipStream_t st = ctx().stream;
        const size_t sn = (size_t)s->n, sm = (size_t)s->m;
        if (s->rcbar.n < sn) { s->rcbar.alloc(sn); s->rx.alloc(sn); s->rax.alloc(sm); s->rpart.alloc(4 * kDgaParts); }
        const bool timed = s->w.timer.on;
        s->w.timer.on = false;
        dga_argmin(s, s->rcbar.p, s->rx.p);
        s->w.timer.on = timed;
        if (s->m > 0) matrix_spmv(s->k, false, s->rx.p, s->rax.p, SLP_ORDER_SEQUENTIAL);
        hipLaunchKernelGGL(k_dga_energy_x, dim3(kDgaParts), dim3(kBlock), 0, st, s->n, s->rcbar.p, s->lb.p, s->ub.p, s->rpart.p);
        hipLaunchKernelGGL(k_dga_energy_y, dim3(kDgaParts), dim3(kBlock), 0, st, s->m, s->m_eq, s->y.p, s->b.p, s->rax.p, s->rpart.p + kDgaParts);
        SLP_HIP(hipGetLastError());
        std::vector<double> h(4 * kDgaParts);
        s->rpart.download(h.data(), h.size());
        dga_report_finish(h.data(), s->m > 0, out);
        dga_read_ctl(s, nullptr);
    })
}

int slp_dga_timing(slp_dga *s, int on) {
    SLP_API_INT({
        SLP_REQUIRE(s, "slp_dga_timing: NULL handle");
        s->w.timer.set(on);
    })
}

int slp_dga_timing_read(slp_dga *s, double out[5]) {
    SLP_API_INT({
        SLP_REQUIRE(s && out, "slp_dga_timing_read: NULL argument");
        s->w.timer.read(out);
    })
}

int slp_dga_line_search(slp_matrix *a, const double *direction, const double *b, const double *c_bar, const double *ub, const double *lb,
                        int path, const double *draws, int64_t ndraws, double out[4]) {
    SLP_API_INT({
        SLP_REQUIRE(a && direction && b && c_bar && ub && lb && out, "slp_dga_line_search: NULL argument");
        SLP_REQUIRE(ndraws >= 0 && (draws || ndraws == 0), "slp_dga_line_search: bad draws");
        const i64 m = a->a.nrow, n = a->a.ncol;
        SLP_REQUIRE(m > 0, "slp_dga_line_search: no rows");
        hipStream_t st = ctx().stream;
        DgaSearch w;
        search_setup(w, n, path);
        search_push_random(w, draws, ndraws);
        DevBuf<double> g, db, dc, dub, dlb;
        g.upload(direction, (size_t)m); db.upload(b, (size_t)m);
        dc.upload(c_bar, (size_t)n); dub.upload(ub, (size_t)n); dlb.upload(lb, (size_t)n);
        // the equality form of the partial results: any non-zero entry (the caller decides whether to search at all)
        hipLaunchKernelGGL(k_dga_grad, dim3(kDgaParts), dim3(kBlock), 0, st, m, (i64)0, m, 0, (const double *)nullptr, db.p,
                           (const double *)nullptr, g.p, w.part_gb.p, w.part_min.p, w.part_any.p);
        search_run(w, a, m, g.p, dc.p, dlb.p, dub.p, 0);
        DgaCtl h;
        w.ctl.download(&h, 1);
        if (!h.active) h.flags |= DGA_EMPTY;   // a zero direction has no breakpoints
        out[0] = h.t;
        out[1] = (double)h.flags;
        out[2] = (double)h.consumed;
        out[3] = (double)h.nb;
    })
}

}  // extern "C"
