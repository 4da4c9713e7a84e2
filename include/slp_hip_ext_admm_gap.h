/*
 * slp_hip_ext_admm_gap.h -- the two single ADMM solvers stop on a certified duality gap: the Gauss-Seidel form (slp_admm,
 * csrc/slp_admm.hip) and the matrix-free conjugate-gradient form (slp_admm_cg, csrc/slp_admm_cg.hip).  Entry points of
 * libslp_hip.so beyond include/slp_hip.h, which stays as it is; include/slp_hip_ext.h brings this header along.  Same
 * conventions: 0 on success, slp_last_error() describes a failure, one host thread per handle.
 *
 * No counterpart in the reference: its lp_admm reports the augmented-Lagrangian energy and two violations and stops on
 * nothing.  The decision and the order of the sums are those of the single Chambolle-Pock solver
 * (include/slp_hip_ext_cp_gap.h; scalar arithmetic csrc/slp_cp_gap.h, slices and fold csrc/slp_gap_fold.h).  What is new is the
 * dual vector: an ADMM multiplier is not dual feasible as it stands, and csrc/slp_admm_gap.h repairs it.
 *
 * A state counts its whole iterations t from 1 over its life, armed or not: the iterate call adds what it ran, and an x-step
 * half followed by a multiplier half is one iteration, which the multiplier half ends.  x_t is lp_admm(nb_iter = t - 1), which
 * runs nb_iter + 1 iterations.  The bench call evaluates nothing and counts nothing.
 *
 * The certificate is defined on the standard form the solver holds: A (m x N, slack columns included), b, c, lb, ub after the
 * set-up chain's row normalisations, x_t (all N entries: the vector the drivers return, not the CG form's projected xp) and
 * lam_t after t whole iterations.  In the forms with an implicit slack column, row i's slack is column n_o + i with the single
 * entry sc_i.  A slack column is a column j with c_j == 0 and exactly one stored entry a_ij: the implicit slack columns by
 * construction; in the explicit forms (slp_admm_create, slp_admm_create_lp, slp_admm_cg_create) they are found from the
 * transposed copy's row lengths at the first evaluation.
 *   yhat_i    = 0 if some slack column j of row i has a_ij lam_i != 0 and min(a_ij lam_i lb_j, a_ij lam_i ub_j) == -inf (the
 *               NaN-propagating minimum), else lam_i.  Any yhat gives a valid bound; this one takes out the -inf a slack
 *               without a bound on the side lam_i pushes to would contribute;
 *   d_j       = c_j + (A^T yhat)_j through the product the solver runs on (CSR walk, strips, value dictionary with deferred
 *               row scaling, chunks); sc_i yhat_i, one product, for an implicit slack column;
 *   primal    = sum_j c_j x_t,j;
 *   bound     = sum_j [d_j != 0 ? min(d_j lb_j, d_j ub_j) : 0] - sum_i [yhat_i != 0 ? yhat_i b_i : 0], a lower bound on the LP's
 *               value; -inf where an original variable has an infinite bound on the side d_j pushes to;
 *   violation = max(max_i |(A x_t)_i - b_i|, max_j (lb_j - x_t,j), max_j (x_t,j - ub_j), 0), NaN-propagating, folded from 0.
 *               It is the violation of the STANDARD FORM in the solver's row-normalised units -- those of the report's
 *               out[1] -- not of the LP in the caller's units;
 *   stop iff violation <= tol_feas and |primal - bound| <= tol_gap (1 + |primal| + |bound|) with a finite left-hand side:
 *   a NaN or an infinite gap never stops (cp_gap_decide).
 *
 * The three sums follow the slice order of include/slp_hip_ext_cp_gap.h: S(count) = 256 min(max(ceil(count / 256), 1), 512)
 * slices, term r in slice r mod S, a slice adds its terms from 0.0 in increasing r, and the same two-stage fold -- primal and
 * the column terms over the stored columns (slp_admm and the explicit CG forms: all N; the implicit CG forms: the n_o original
 * variables), yhat.b over this rank's m rows; the violation is a maximum, exact in any order.  An implicit slack column belongs
 * to its row: the row's slice adds yhat_i b_i and then subtracts the slack column's term (bound = columns - rows), and takes the
 * slack's bound violations; its cost is 0 by construction, so it has no part in primal.
 *
 * Under a communicator (CG form: rows and their slack columns partitioned, original variables replicated) every rank calls
 * the same entry points and takes the same decision from the reduced numbers.  The slice count of the column pass depends on
 * n_o alone, so primal and the original columns' terms are added in the same order, from the same all-reduced A^T yhat (one
 * all-reduce of n_o doubles on the compute stream), on every rank: the same bits.  yhat and the slack columns' terms are
 * rank-local; the row sums (yhat.b minus the slack columns' terms) are summed and the violation maxed over the ranks on the
 * host.
 */
#ifndef SLP_HIP_EXT_ADMM_GAP_H
#define SLP_HIP_EXT_ADMM_GAP_H

#include <stdint.h>

#include "slp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[0..2] = primal, bound, violation of the current iterate, to be called between whole iterations (an error between an
 * x-step half and its multiplier half).  Changes nothing: neither x, xp, lambda nor the iteration count, the armed test or its
 * record, nor any buffer an iteration or its captured graph uses (it writes buffers of its own, allocated at the first
 * evaluation; the CG form first gathers slices that are stale under sharded updates).  Synchronises. */
int slp_admm_certificate(slp_admm *s, double out[3]);
int slp_admm_cg_certificate(slp_admm_cg *s, double out[3]);

/* tol_gap, tol_feas >= 0 and finite with check_every >= 1 arm the test; tol_gap < 0 disarms; anything else is an error and
 * leaves the state as it was, and so does a call between the two halves of an iteration.  Either way a stopped state runs again.
 * On an armed state the iterate call cuts its k iterations at the iterations t with t % check_every == 0, runs every piece
 * exactly as an unarmed state does (the same captured graph or the same eager launches: x, xp and lambda after t iterations
 * are bit for bit the unarmed state's, at every reuse level and either x-step), and after a check iteration evaluates the
 * certificate outside any captured graph, reads four doubles back (one synchronising read per check) and decides on the host.
 * The multiplier half step does the same when it ends a check iteration.  Once stopped, the state stays stopped until this is
 * called again: the iterate call and the two half steps enqueue nothing and t stays.  A state that was never armed launches
 * exactly what it launched before these entry points existed. */
int slp_admm_set_stop_gap(slp_admm *s, double tol_gap, double tol_feas, int64_t check_every);
int slp_admm_cg_set_stop_gap(slp_admm_cg *s, double tol_gap, double tol_feas, int64_t check_every);

/* Iterations completed (t), 1 = stopped, and primal, bound, violation of the last certificate a check evaluated (+inf, -inf,
 * +inf before the first).  Any pointer may be NULL. */
int slp_admm_gap_state(slp_admm *s, int64_t *iterations, int32_t *stopped, double *primal, double *bound, double *violation);
int slp_admm_cg_gap_state(slp_admm_cg *s, int64_t *iterations, int32_t *stopped, double *primal, double *bound, double *violation);

/* The rest of the CG form's iterate: the first `count` entries of the projected xp (under sharded updates a collective: every
 * rank calls it), and this rank's m multipliers. */
int slp_admm_cg_get_xp(slp_admm_cg *s, double *xp, int64_t count);
int slp_admm_cg_get_lambda(slp_admm_cg *s, double *lam);

#ifdef __cplusplus
}
#endif
#endif /* SLP_HIP_EXT_ADMM_GAP_H */
