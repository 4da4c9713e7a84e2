/*
 * slp_hip_ext_admm_batch.h -- the entry points of libslp_hip.so for per-instance stopping of the batched ADMM solver.
 * Included by include/slp_hip_ext.h, so whoever includes that header has these too; a file of its own, so that the text of
 * slp_hip_ext.h keeps declaring the two entry points of the batched Chambolle-Pock solver and nothing else.
 * Same conventions as include/slp_hip.h: plain pointers and sizes, 0 on success, slp_last_error() describes a failure,
 * one host thread per handle.
 */
#ifndef SLP_HIP_EXT_ADMM_BATCH_H
#define SLP_HIP_EXT_ADMM_BATCH_H

#include <stdint.h>

#include "slp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched ADMM: stop each instance on its residual and its step ---------- *
 * No counterpart in the reference (no stopping test, one LP per call).  The rule is that of slp_many_admm_set_stop, per
 * instance of the batch; the batch semantics are those of slp_cp_batch_set_stop_gap.  The state counts its whole iterations
 * t from 1 over its life, armed or not; an iteration is the right-hand side, the sweep that gives x_t (all N = n + m_ineq
 * columns of the standard form) and the multiplier update that gives lambda_t.  At the end of an iteration t with
 * t % check_every == 0 every running instance evaluates
 *   residual_t = max_i |(A x_t)_i - b_i| over the m rows of the standard form, with the very (A x)_i - b_i the multiplier
 *                update forms (0 for m = 0);
 *   step_t     = max_j |x_t,j - x_{t-1},j| over all N columns, slacks included, x_0 the stored start: new minus old in the
 *                sweep, which visits every row of M exactly once per iteration,
 * both exact and as np.max (a NaN stays), and stops iff residual_t <= tol_residual and step_t <= tol_step: a NaN never
 * stops.  A stopped instance keeps x_t and lambda_t -- bit for bit those of lp_admm(..., nb_iter = t - 1,
 * order = ORDER_SEQUENTIAL) -- while the others go on, their iterates unchanged by the test: from the first arming on the
 * state launches kernels in which a lane of a stopped instance returns before its first load.  The batch has ONE iteration
 * counter, so unlike an LP of slp_many_admm_set_stop a stopped instance stays stopped for the life of the state: a further
 * call changes tolerances and cadence for the running instances and keeps the flags; tol_residual < 0 turns the test off --
 * the running instances go on untested, the stopped ones stay as they are (on a state that was never armed it changes
 * nothing).  tol_residual, tol_step >= 0 and finite with check_every >= 1 arm the test; anything else is an error, and so is
 * a call between slp_admm_batch_sweep_step and slp_admm_batch_multiplier_step.  The test's buffers are allocated at the
 * first arming; a state that was never armed launches the kernels without the test.  Synchronises.
 * On an armed state slp_admm_batch_iterate and slp_admm_batch_multiplier_step first read how many instances still run (one
 * synchronising read) and enqueue nothing, and leave t unchanged, when none does; the test is evaluated on the device inside
 * (tile form) or behind (levels form) the launches of a check iteration and nothing else is read back, so the stopping
 * iteration does not depend on how a run is split into calls.  slp_admm_batch_sweep_step followed by
 * slp_admm_batch_multiplier_step is one iteration: the step of a check iteration waits in the instance's record for the
 * multiplier half, which ends it.  slp_admm_batch_bench evaluates no test. */
int slp_admm_batch_set_stop(slp_admm_batch *s, double tol_residual, double tol_step, int64_t check_every);
/* Per instance: iterations completed (t; for a stopped instance its stopping iteration), 1 = stopped, and the last
 * evaluated residual and step (+inf before the first test).  batch values each; any pointer may be NULL.  Synchronises. */
int slp_admm_batch_stop_state(slp_admm_batch *s, int64_t *iterations, int32_t *stopped, double *residual, double *step);

#ifdef __cplusplus
}
#endif
#endif /* SLP_HIP_EXT_ADMM_BATCH_H */
