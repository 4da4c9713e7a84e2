/*
 * slp_hip_ext.h -- entry points of libslp_hip.so beyond include/slp_hip.h, which stays as it is (its 215 entry points
 * are what existing callers bind).  Same conventions: plain pointers and sizes, 0 on success, slp_last_error()
 * describes a failure, one host thread per handle, reference citations are file:line under the reference tree's
 * pysparselp/.
 */
#ifndef SLP_HIP_EXT_H
#define SLP_HIP_EXT_H

#include <stdint.h>

#include "slp_hip.h"
/* per-instance stopping of the batched ADMM solver: declared in a header of its own, which this one brings along */
#include "slp_hip_ext_admm_batch.h"
/* per-instance stopping of the batched dual gradient ascent: likewise */
#include "slp_hip_ext_dga_batch.h"
/* a cut-off for the bound of each LP of the dual-ascent list solver: likewise */
#include "slp_hip_ext_dga_many.h"
/* the dual-ascent list solver over the list of its live LPs (compaction): likewise */
#include "slp_hip_ext_dga_many_live.h"
/* the Chambolle-Pock and the ADMM list solver over the lists of their live LPs (compaction): likewise */
#include "slp_hip_ext_many_live.h"
/* per-instance right-hand sides of the batched dual ascent and the batched ADMM solver: likewise */
#include "slp_hip_ext_batch_rhs.h"
/* which packet form a tall-cell product copy has: likewise */
#include "slp_hip_ext_tall.h"
/* the single Chambolle-Pock solver stops on a certified duality gap: likewise */
#include "slp_hip_ext_cp_gap.h"
/* the two single ADMM solvers (Gauss-Seidel and matrix-free CG) stop on a certified duality gap: likewise */
#include "slp_hip_ext_admm_gap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched Chambolle-Pock: stop each instance on a certified duality gap -- *
 * No counterpart in the reference: it evaluates the same bound (energy2, ChambollePockPPD.py:262-266) at its reports only,
 * stops on nothing and solves one LP per call.  The certificate is that of slp_many_cpgap_set_stop, per instance of the
 * batch.  The state counts its whole iterations t from 1 over its life, armed or not.  With K = [A_eq; A_ineq], x_t and
 * y_t = [y_eq; y_ineq] of an instance after t whole iterations, at the end of an iteration t with t % check_every == 0
 * every running instance evaluates
 *   d_j       = c_j + (K^T y_t)_j, the bits the next primal half computes;
 *   primal    = sum_j c_j x_t,j;
 *   bound     = sum_j [d_j != 0 ? min(d_j lb_j, d_j ub_j) : 0] - sum_r [y_r != 0 ? y_r b_r : 0], a lower bound on the LP's
 *               value (y_t is dual feasible by construction), -inf where a free variable has d_j of the wrong sign;
 *   violation = max(max_{r < m_eq} |(K x_t)_r - b_r|, max_{r >= m_eq} ((K x_t)_r - b_r), 0), exact, NaN-propagating,
 * and stops iff violation <= tol_feas and |primal - bound| <= tol_gap (1 + |primal| + |bound|) with |primal - bound|
 * finite: a NaN or an infinite gap never stops.  The two sums are in the fixed order of slp_cp_batch_report (entry r in
 * slice r mod S, a slice in increasing r, then the slices in increasing order), a function of the shapes only.
 * A stopped instance keeps its x, z, y, x4 after its t iterations -- bit for bit those of the batch without a test after t
 * iterations -- while the others go on: from the first arming on the state launches kernels in which a lane of a stopped
 * instance returns before its first load.  The batch has ONE iteration counter, so unlike an LP of slp_many_cpgap_set_stop
 * a stopped instance stays stopped for the life of the state: a further call changes tolerances and cadence for the
 * running instances and keeps the flags; tol_gap < 0 turns the test off -- the running instances go on untested, the
 * stopped ones stay as they are (on a state that was never armed it changes nothing).  tol_gap, tol_feas >= 0 and finite
 * with check_every >= 1 arm the test; anything else is an error.  The test's buffers are allocated at the first arming.
 * To be called between whole iterations.  Synchronises.
 * On an armed state slp_cp_batch_iterate and slp_cp_batch_dual_step first read how many instances still run (one
 * synchronising read) and enqueue nothing, and leave t unchanged, when none does; the certificate is enqueued behind the
 * dual half of a check iteration and nothing else is read back.  slp_cp_batch_primal_step followed by
 * slp_cp_batch_dual_step is one iteration: the dual half ends it.  slp_cp_batch_bench evaluates no certificate. */
int slp_cp_batch_set_stop_gap(slp_cp_batch *s, double tol_gap, double tol_feas, int64_t check_every);
/* Per instance: iterations completed (t; for a stopped instance its stopping iteration), 1 = stopped, and primal, bound,
 * violation of the last evaluated certificate (+inf, -inf, +inf before the first).  batch values each; any pointer may be
 * NULL.  Synchronises. */
int slp_cp_batch_gap_state(slp_cp_batch *s, int64_t *iterations, int32_t *stopped, double *primal, double *bound, double *violation);

#ifdef __cplusplus
}
#endif
#endif /* SLP_HIP_EXT_H */
