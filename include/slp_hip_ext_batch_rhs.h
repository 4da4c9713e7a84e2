/*
 * slp_hip_ext_batch_rhs.h -- the entry points of libslp_hip.so for per-instance right-hand sides of the batched dual
 * gradient ascent and of the batched ADMM solver.  Included by include/slp_hip_ext.h, so whoever includes that header has
 * these too; a file of its own, so that the other headers keep their text.  Same conventions as include/slp_hip.h: plain
 * pointers and sizes, 0 on success, slp_last_error() describes a failure, one host thread per handle.
 */
#ifndef SLP_HIP_EXT_BATCH_RHS_H
#define SLP_HIP_EXT_BATCH_RHS_H

#include <stdint.h>

#include "slp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- right-hand sides per instance ------------------------------------------ *
 * No counterpart in the reference (one LP per call).  Both constructors take one right-hand side for all instances; these
 * calls replace it, by one vector for all (*_batched = 0, replicated by the library) or by one row per instance
 * ([batch x rows], row-major, *_batched = 1).  Instance k is then bit for bit what the single solver computes on a copy of
 * the LP whose right-hand sides are row k.  Both are allowed only while the state has completed no iteration and no half
 * iteration (slp_admm_batch_sweep_step, slp_admm_batch_multiplier_step); afterwards they fail and change nothing.  They may
 * be called more than once before the first iteration.  The extra device memory -- 8 m Bp bytes for a batched b, and for
 * ADMM 8 N Bp bytes more for each of lb / ub that becomes batched only because its slack part now differs per instance, Bp
 * the padded batch -- is checked against slp_device_memory plus the cached blocks before anything is allocated; a refusal
 * leaves the state usable with the right-hand sides it had.  A state that never calls them launches what it launched
 * before they existed.  Both synchronise.
 *
 * Dual ascent: b is [m] or [batch x m] over the rows of K = [A_eq; A_ineq].  It enters the gradient (K x - b, g . b) and
 * the y . b chain of the energy, each instance through b + k * stride, stride 0 for a shared vector; whether an instance's
 * start is frozen (dual energy -inf) is derived again. */
int slp_batch_dga_set_rhs(slp_batch_dga *s, const double *b, int b_batched);
/* ADMM: the arrays are in the units of slp_admm_batch_create_lp (unscaled); b_eq is [m_eq] or [batch x m_eq], b_lower and
 * b_upper [m_ineq] or [batch x m_ineq].  A NULL pointer keeps what the state was created with (or was last given).  The
 * library builds, on the device and per instance, what the single set-up chain produces for that instance's LP: b_eq
 * scaled by the equality block's row scaling and then by the stacked system's (use_preconditioning), 0 on the inequality
 * rows; b_lower / b_upper scaled by the inequality block's row scaling as the slack part of lb / ub (-inf / +inf stay);
 * A^T b_k by the set-up's product in SLP_ORDER_SEQUENTIAL and q_k = -c_k + gamma_eq A^T b_k.  The start does not depend on
 * the right-hand sides and stays. */
int slp_admm_batch_set_rhs(slp_admm_batch *s, const double *b_eq, int b_eq_batched, const double *b_lower, int b_lower_batched,
                           const double *b_upper, int b_upper_batched);

#ifdef __cplusplus
}
#endif
#endif /* SLP_HIP_EXT_BATCH_RHS_H */
