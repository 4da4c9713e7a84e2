/*
 * slp_hip_ext_dga_batch.h -- the entry points of libslp_hip.so for per-instance stopping of the batched dual gradient ascent.
 * Included by include/slp_hip_ext.h, so whoever includes that header has these too; a file of its own, so that the text of
 * slp_hip_ext.h keeps declaring the two entry points of the batched Chambolle-Pock solver and nothing else.
 * Same conventions as include/slp_hip.h: plain pointers and sizes, 0 on success, slp_last_error() describes a failure,
 * one host thread per handle.
 */
#ifndef SLP_HIP_EXT_DGA_BATCH_H
#define SLP_HIP_EXT_DGA_BATCH_H

#include <stdint.h>

#include "slp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched dual gradient ascent: stop each instance on its step or on a cut-off for its bound ---------- *
 * No counterpart in the reference (a fixed number of iterations, one LP per call).  The step rule is that of
 * slp_many_dual_set_stop, per instance of the batch; the bound rule is new.  The state counts its iterations t from 1 over
 * its life, armed or not, the same number for every instance that moves.  At the end of an iteration t with
 * t % check_every == 0 every instance that is neither frozen nor stopped evaluates
 *   step_t  = max_r |y_t,r - y_{t-1},r| over all m multipliers (the inequality part after its clamp), as np.max (a NaN
 *             stays); a kind of rows whose block predicate was off in iteration t contributes 0;
 *   bound_t = the dual energy of y_t, bit for bit out[3 k] of slp_batch_dga_report after t iterations -- a certified lower
 *             bound on the instance's LP value; evaluated only when cut-offs are given,
 * and stops iff step_t <= tol (when tol >= 0) or bound_t >= targets[k] (when targets is given and targets[k] < +inf): both
 * are looked at, so the reason may name both.  A NaN in either quantity never stops, nor does an instance whose status
 * carries the NaN bit.  A stopped instance keeps y_t, the x of the top of iteration t -- bit for bit the single solve of
 * its data after t iterations --, its tie-draw count and its flags, and takes no part in any later launch: no column or
 * row pass, an empty sort segment, no search, no update, and it no longer holds the front of the stream of tie draws, whose
 * draws behind it may be dropped.  Hence it cannot be resumed: no call clears a stopped mark.  The others go on, their
 * iterates unchanged by the test.  slp_batch_dga_frozen keeps meaning "dual-infeasible start": 0 for a stopped instance.
 *
 * tol < 0 turns the step test off, targets == NULL the bound test (else `batch` values; +inf: this instance has no cut-off;
 * a NaN or -inf is refused); with both off the whole test is off and the launches are those of a state that was never
 * armed, while stopped instances stay stopped.  tol must be finite, check_every >= 1.  A further call changes the rule for
 * the instances still moving.  The test's buffers are allocated at the first arming.  Synchronises.
 * On a state that was ever armed slp_batch_dga_iterate first reads the controls (one synchronising read) and enqueues
 * nothing, leaving the iteration count, when every instance is frozen or stopped; the test itself runs on the device behind
 * the update passes of a check iteration and nothing else is read back, so a stopping iteration does not depend on how a
 * run is split into calls. */
int slp_batch_dga_set_stop(slp_batch_dga *s, double tol, const double *targets, int64_t check_every);
/* Per instance: iterations completed (for a stopped instance its stopping iteration, 0 for a frozen one), the reason as a
 * bit mask (0 = moving or frozen, 1 = step, 2 = bound, 3 = both), and the last evaluated step and bound (+inf and -inf
 * before the first evaluation; -inf is always a valid lower bound).  The step is evaluated at every check, the bound at the
 * checks with cut-offs.  batch values each; any pointer may be NULL.  Synchronises. */
int slp_batch_dga_stop_state(slp_batch_dga *s, int64_t *iterations, int32_t *reason, double *step, double *bound);

#ifdef __cplusplus
}
#endif
#endif /* SLP_HIP_EXT_DGA_BATCH_H */
