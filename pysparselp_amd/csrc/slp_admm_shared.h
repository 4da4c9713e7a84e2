// slp_admm_shared.h -- what slp_admm.hip shares with the batched solver (slp_admm_batch.hip) and the list solver
// (slp_admm_many.hip): the set-up chain of lp_admm (ADMM.py:73-101) and a view of the state it leaves.  The batched solver reads
// what depends on the constraints only; the list solver, whose composite LP carries every LP's own vectors, also c, q and xp0.
#pragma once
#include <vector>

#include "slp_common.h"

struct slp_admm;

namespace slp {

// Views into a state created by admm_create_lp; they live as long as the state.  The Gauss-Seidel plan of M is its level-ordered
// copy: position t holds row gs_rows[t], entries gs_ptr[t] .. gs_ptr[t + 1], gs_invd[t] = 1 / M[row, row]; level l is the
// positions lptr[l] .. lptr[l + 1] (levels_only: no band reorders them).
struct AdmmShared {
    slp_matrix *a = nullptr;   // the standard-form, row-normalised A (m x N) with its transposed copy
    i64 N = 0, m = 0;
    const double *b = nullptr, *lb = nullptr, *ub = nullptr;   // [m], [N], [N]: stacked and scaled (:76-91)
    const double *x0 = nullptr;                                // [N] = [x0; A_ineq x0] (:84-86)
    const double *atb = nullptr;                               // [N] A^T b (:95)
    const double *c = nullptr, *q = nullptr, *xp0 = nullptr;   // [N] [c; 0], (-c) + gamma_eq A^T b (:97), max(x0, 0) (:98)
    // the row scalings the chain applied (:76-83, :90-91): [m_eq] (NULL without an equality block), [m - m_eq], [m] (NULL without
    // use_preconditioning); slp_admm_batch_set_rhs brings an instance's own right-hand sides to the state's units with them
    i64 m_eq = 0;
    const double *scale_eq = nullptr, *scale_ineq = nullptr, *scale_rows = nullptr;
    i64 nlevels = 0, max_width = 0, nnz_m = 0;
    std::vector<i64> lptr;
    const i64 *gs_ptr = nullptr;
    const i32 *gs_idx = nullptr, *gs_rows = nullptr;
    const double *gs_val = nullptr, *gs_invd = nullptr;
};

// slp_admm_create_lp (throws instead of returning NULL).  scaled_ineq != NULL receives the row-normalised inequality block
// (owned by the caller), with which x0's slack part was formed.  levels_only: M's Gauss-Seidel plan is the level-ordered copy alone --
// the rows of a level contiguous (bands reorder the rows inside their runs), no lane records of the single-workgroup sweeps.
// earliest_levels: the plan moves no sink rows to a level of their own (GsPlan::earliest_levels), whatever their number.
slp_admm *admm_create_lp(int64_t n, int64_t m_eq, const int64_t *eq_indptr, const int32_t *eq_indices, const double *eq_data,
                         const double *b_eq, int64_t m_ineq, const int64_t *in_indptr, const int32_t *in_indices,
                         const double *in_data, const double *b_lower, const double *b_upper, const double *c, const double *lb,
                         const double *ub, const double *x0, double gamma_eq, double gamma_ineq, int use_preconditioning, int order,
                         slp_matrix **scaled_ineq, bool levels_only, bool earliest_levels = false);

// Fills the view of a state created with levels_only.
void admm_shared(slp_admm *s, AdmmShared *v);

}  // namespace slp
