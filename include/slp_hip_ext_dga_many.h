/*
 * slp_hip_ext_dga_many.h -- the entry points of libslp_hip.so for stopping each LP of the dual-ascent list solver on a cut-off
 * for its bound.  Included by include/slp_hip_ext.h, so whoever includes that header has these too; a file of its own, so that
 * the text of slp_hip.h (which declares slp_many_dual_set_stop and slp_many_dual_stop_state) and of slp_hip_ext.h stays as it is.
 * Same conventions as include/slp_hip.h: plain pointers and sizes, 0 on success, slp_last_error() describes a failure,
 * one host thread per handle.
 */
#ifndef SLP_HIP_EXT_DGA_MANY_H
#define SLP_HIP_EXT_DGA_MANY_H

#include <stdint.h>

#include "slp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dual gradient ascent on a list of LPs: stop each LP on its step or on a cut-off for its bound ---------- *
 * No counterpart in the reference (a fixed number of iterations, one LP per call).  The step rule is that of
 * slp_many_dual_set_stop; the bound rule is that of slp_batch_dga_set_stop (slp_hip_ext_dga_batch.h), per LP of the list.
 * Iterations of an LP count from 1 over its whole life.  At the end of an iteration t with t % check_every == 0 every LP that
 * is neither frozen nor stopped evaluates, inside the iteration kernel,
 *   step_t  = max_r |y_t,r - y_{t-1},r| over all its multipliers (the inequality part after its clamp), as np.max (a NaN
 *             stays); a kind of rows whose block predicate was off in iteration t contributes 0;
 *   bound_t = the dual energy of y_t, bit for bit out[3 k] of slp_many_dga_report after t iterations -- a certified lower
 *             bound on the LP's value; evaluated only when cut-offs are given, and then at every check of every moving LP,
 * and stops iff step_t <= tol (when tol >= 0) or bound_t >= targets[k] (when targets is given and targets[k] < +inf): both
 * are looked at, so the reason may name both.  A NaN in either quantity never stops, nor does an LP whose status carries
 * the NaN bit.  A stopped LP keeps y_t, the x and c_bar of the top of iteration t -- bit for bit the single solve of its
 * data after t iterations --, its tie-draw count and its flags, and takes no part in any later launch; the draws behind it
 * may be dropped.  Hence it cannot be resumed: no call clears a stopped mark.  The others go on, their iterates unchanged
 * by the test.
 *
 * tol < 0 turns the step test off, targets == NULL the bound test (else `count` values; +inf: this LP has no cut-off; a NaN
 * or -inf is refused); with both off the whole test is off and the launches are those of a state that was never armed,
 * while stopped LPs stay stopped.  tol must be finite, check_every >= 1.  With cut-offs an LP of more than 65536 rows is
 * refused, before anything is launched: up to there a lane of the report's reductions holds at most one term, which is what
 * makes the kernel's bound the report's bit for bit.  A further call changes the rule for the LPs still moving, from their
 * next check iteration.  slp_many_dual_set_stop(s, tol, k) is slp_many_dual_set_cutoff(s, tol, NULL, k).  Synchronises. */
int slp_many_dual_set_cutoff(slp_many_dga *s, double tol, const double *targets, int64_t check_every);
/* Per LP: iterations completed (for a stopped LP its stopping iteration, 0 for a frozen one), the reason as a bit mask
 * (0 = moving or frozen, 1 = step, 2 = bound, 3 = both), and the last evaluated step and bound (+inf and -inf before the
 * first evaluation; -inf is always a valid lower bound).  The step is evaluated at every check, the bound at the checks
 * with cut-offs.  slp_many_dual_stop_state's `stopped` is reason != 0.  count values each; any pointer may be NULL.
 * Synchronises. */
int slp_many_dual_cutoff_state(slp_many_dga *s, int64_t *iterations, int32_t *reason, double *step, double *bound);

#ifdef __cplusplus
}
#endif
#endif /* SLP_HIP_EXT_DGA_MANY_H */
