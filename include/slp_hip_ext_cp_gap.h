/*
 * slp_hip_ext_cp_gap.h -- the single Chambolle-Pock solver (slp_cp, csrc/slp_cp.hip) stops on a certified duality gap.
 * Entry points of libslp_hip.so beyond include/slp_hip.h, which stays as it is; include/slp_hip_ext.h brings this header
 * along.  Same conventions: 0 on success, slp_last_error() describes a failure, one host thread per handle.
 *
 * No counterpart in the reference: it evaluates the same bound (energy2, ChambollePockPPD.py:262-266) at its reports only
 * and stops on nothing.  The certificate is the one the batched and the list solver stop on, its scalar arithmetic shared
 * through csrc/slp_cp_gap.h, here on every copy a state can run on: ELL, CSR, strips, value dictionary, tall cells,
 * chunks, with or without the CSR arrays, and row-partitioned over the ranks of a communicator.
 *
 * The state counts its whole iterations t from 1 over its life, armed or not: the iterate call adds what it ran, and a
 * primal half step followed by a dual half step is one iteration, which the dual half ends.  The bench call evaluates
 * nothing and counts nothing.
 *
 * With K = [A_eq; A_ineq] one-sided, b, c, lb, ub as the state holds them, x_t (the iterate, not the extrapolated z) and
 * y_t = [y_eq; y_ineq] after t whole iterations:
 *   d_j       = c_j + (K^T y_t)_j in the bits of the next primal half: (c + s_eq) + s_ineq where the LP has both kinds of
 *               rows on one GPU -- the CSR or ELL walk's two chains, the two products over the copies of A_eq^T / A_ineq^T,
 *               or the two masked products, whichever the state's split form is; under a communicator the partial K^T y
 *               is all-reduced once (n doubles, on the compute stream) as in an iteration;
 *   primal    = sum_j c_j x_t,j;
 *   bound     = sum_j [d_j != 0 ? min(d_j lb_j, d_j ub_j) : 0] - sum_r [y_r != 0 ? y_r b_r : 0], a lower bound on the LP's
 *               value (y_t is dual feasible by construction), -inf where a free variable has d_j of the wrong sign;
 *   violation = max(max_{r < m_eq} |(K x_t)_r - b_r|, max_{r >= m_eq} ((K x_t)_r - b_r), 0), NaN-propagating;
 *   stop iff violation <= tol_feas and |primal - bound| <= tol_gap (1 + |primal| + |bound|) with a finite left-hand side:
 *   a NaN or an infinite gap never stops.
 *
 * The order of the three sums is a function of n, m and the rank's row block only, never of the matrix format.  A vector
 * of `count` terms (the n columns; the rows of this rank) has S(count) = 256 min(max(ceil(count / 256), 1), 512) slices;
 * term r belongs to slice r mod S and a slice adds its terms from 0.0 in increasing r.  They are folded in two
 * stages.  First the slices 256 q .. 256 q + 255 are added, one per lane of a workgroup of 256: a wavefront adds its 64 lanes
 * by halving (lane i += lane i + 32, then 16, 8, 4, 2, 1), and the four wavefronts' sums are added in increasing order.  Then
 * one workgroup of 256 lanes adds these at most 512 sums: lane l adds the sums l and l + 256 from 0.0, then the same tree.  primal and
 * the column terms run over the n columns, y.b over the rank's rows; the violation is folded from 0 the same way (a
 * maximum is exact in any order).  Given the same x, y and d every format returns the same three numbers.  Under a
 * communicator d, primal and the column terms are replicated, y.b is summed and the violation maxed over the ranks on the
 * host, and the decision is taken from the reduced numbers, the same on every rank.
 */
#ifndef SLP_HIP_EXT_CP_GAP_H
#define SLP_HIP_EXT_CP_GAP_H

#include <stdint.h>

#include "slp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[0..2] = primal, bound, violation of the current iterate, to be called between whole iterations.  Changes nothing:
 * neither x, z, y nor the iteration count, the armed test or its record (it writes scratch of the two half steps only).
 * Under a communicator every rank calls it (one all-reduce of n doubles and two scalar reductions).  Synchronises. */
int slp_cp_certificate(slp_cp *s, double out[3]);

/* tol_gap, tol_feas >= 0 and finite with check_every >= 1 arm the test; tol_gap < 0 disarms; anything else is an error
 * and leaves the state as it was.  Either way a stopped state runs again.  On an armed state the iterate call cuts its k
 * iterations at the iterations t with t % check_every == 0, runs every piece exactly as an unarmed state does (the same
 * captured graph or the same eager launches: x, z, y after t iterations are bit for bit the unarmed state's), and after a
 * check iteration evaluates the certificate outside any captured graph, reads the three numbers back (one synchronising
 * read per check) and decides on the host.  The dual half step does the same when it ends a check iteration.  Once
 * stopped, the state stays stopped until this is called again: the iterate call and the two half steps enqueue nothing
 * and t stays.  An unarmed state launches exactly what it launched before this entry point existed.  The certificate's
 * partial sums are allocated at the first evaluation. */
int slp_cp_set_stop_gap(slp_cp *s, double tol_gap, double tol_feas, int64_t check_every);

/* Iterations completed (t), 1 = stopped, and primal, bound, violation of the last certificate a check evaluated (+inf,
 * -inf, +inf before the first).  Any pointer may be NULL. */
int slp_cp_gap_state(slp_cp *s, int64_t *iterations, int32_t *stopped, double *primal, double *bound, double *violation);

#ifdef __cplusplus
}
#endif
#endif /* SLP_HIP_EXT_CP_GAP_H */
