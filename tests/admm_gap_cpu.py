"""numpy restatement of the duality-gap certificate of the single ADMM solvers (include/slp_hip_ext_admm_gap.h), on the
standard-form arrays of ``oracle.admm_setup``: ``A`` (m x N, slack columns stored), ``b``, ``c``, ``lb``, ``ub``.

``yhat_i``     0 if some slack column j of row i (``c_j == 0``, one stored entry ``a_ij``) has ``p = a_ij * lam_i != 0`` and
               ``min(p * lb_j, p * ub_j) == -inf``, else ``lam_i``;
``d``          ``c + A^T yhat``; a slack column's ``d`` is the single product ``a_ij * yhat_i``, as on the device;
``bound``      ``sum_j [d_j != 0 ? min(d_j lb_j, d_j ub_j) : 0] - sum_i [yhat_i != 0 ? yhat_i b_i : 0]``;
``primal``     ``sum_j c_j x_j``;
``violation``  ``max(max_i |(A x)_i - b_i|, max_j (lb_j - x_j), max_j (x_j - ub_j), 0)``, a NaN stays.

The sums are taken in ``np.longdouble`` (u_ld = 2^-64, whose own error is three orders below the tolerances) as the exact
value of the terms as rounded; the tolerances hold for ANY order of summation in fp64, with u = 2^-53 and L the longest column:

  bound      each ``d_j`` is a sum of at most L + 1 terms, each a rounded product: ``|d_j - exact| <= (L + 2) u (|c_j| + sum_i
             |a_ij yhat_i|)`` to first order, and it enters its term multiplied by a bound of magnitude ``max(|lb_j|, |ub_j|)``
             (finite where the term is); the N + m terms are then added in some order: ``(N + m + 2) u (sum|term_j| + sum|yhat_i
             b_i|)`` covers that sum and the terms' own roundings.  1.01 absorbs the second-order terms.
  primal     ``1.01 u (N + 1) sum|c_j x_j|``
  violation  the largest ``oracle.row_error_bound`` of a row (a maximum is exact; ``lb - x`` and ``x - ub`` are single roundings
             of the same operands on both sides, hence equal).

These are derived, not tuned: a dropped wave, slice or term is orders of magnitude above them.

The forms with an implicit slack column (``ADMMCGLPState``, ``DeviceADMM``) hold the same standard form -- plus a slack column
with entry 0 and box [0, 0] per equality row, which contributes nothing -- but normalise its rows on the device, in another
order of summation or as a deferred scaling ``diag(rs) A0``.  ``Restatement.at(..., scale_eps=scale_eps(r))`` widens the tolerances
for that: per normalisation pass a row norm is the square root of a sum of at most ``Lr + 1`` squares in some order (relative
error at most ``(Lr + 2) u``), then one division and one product (``2 u``), and there are two passes, so every stored entry,
right-hand side, slack entry and scaled slack bound of the device is within ``2 (Lr + 4) u`` relative of the oracle's; a deferred
scaling applied after the row sum instead of before it is within the same again.  With ``eps = 4 (Lr + 4) u``, ``Lr`` the longest
row: ``d_j`` moves by at most ``eps sum_i |a_ij yhat_i|`` and its term by that times the bound's magnitude, a term with a scaled
slack bound and every ``yhat_i b_i`` by ``eps`` relative; ``(A x)_i - b_i`` by ``eps ((|A| |x|)_i + |b_i|)`` and a slack's bound
violation by ``eps`` times the bound.

``HIGHS_SLACK`` is NOT derived: HiGHS returns its optimum to its own feasibility tolerances (1e-7), and ``1e-6 (1 + |optimum|)``
leaves room for them wherever a bound is compared with that optimum.
"""
import collections

import numpy as np

from oracle import oracle

U = 2.0 ** -53
HIGHS_SLACK = 1e-6   # relative; see the docstring: HiGHS's own accuracy, not a derived figure
Numbers = collections.namedtuple("Numbers", "primal bound violation tol_primal tol_bound tol_violation repaired")


def setup_of(problem, **kw):
    """``oracle.admm_setup`` on the 8-tuple ``problem``."""
    return oracle.admm_setup(*problem, **kw)


def iterates(problem, nb_iter, every=1, **kw):
    """``{t: (x_t, lam_t)}`` of ``oracle.lp_admm`` for the whole iterations ``t = every, 2 every, ... <= nb_iter``: all N entries of
    ``x`` after the sweep of iteration t and the multipliers after its update (the hook sees them at the next sweep)."""
    xs, lams = {}, {}

    def hook(i, _, x, lam):
        xs[i + 1] = x.copy()
        lams[i] = lam.copy()

    oracle.lp_admm(*problem, nb_iter=nb_iter, iterate_hook=hook, **kw)   # sweeps i = 0 .. nb_iter: lam_t for t <= nb_iter
    return {t: (xs[t], lams[t]) for t in range(every, nb_iter + 1, every)}


class Restatement:
    """The certificate on one standard form; the index work is done once."""

    def __init__(self, setup):
        a = oracle.as_csr(setup["a"])
        self.a = a
        self.m, self.N = a.shape
        self.b, self.c, self.lb, self.ub = (np.asarray(setup[k], dtype=np.float64) for k in ("b", "c", "lb", "ub"))
        self.indptr, self.cols, self.vals = np.asarray(a.indptr), np.asarray(a.indices, dtype=np.int64), np.asarray(a.data, dtype=np.float64)
        self.rows = np.repeat(np.arange(self.m), np.diff(self.indptr))
        counts = np.bincount(self.cols, minlength=self.N)
        self.slack = (self.c == 0.0) & (counts == 1)
        self.longest_column = int(counts.max()) if counts.size else 0
        self.slack_entry = self.slack[self.cols]   # per stored entry: it is the one entry of a slack column
        self.longest_row = int(np.diff(self.indptr).max()) if self.m else 0

    def yhat(self, lam):
        """``(yhat, number of repaired multipliers)``."""
        e = np.nonzero(self.slack_entry)[0]
        with np.errstate(invalid="ignore", over="ignore"):
            p = self.vals[e] * lam[self.rows[e]]
            j = self.cols[e]
            lo = np.minimum(p * self.lb[j], p * self.ub[j])   # np.minimum propagates a NaN, like nan_min
            bad = (p != 0.0) & (lo == -np.inf)
        repaired = np.zeros(self.m, dtype=bool)
        repaired[self.rows[e[bad]]] = True
        return np.where(repaired, 0.0, lam), int(repaired.sum())

    def at(self, x, lam, scale_eps=0.0):
        """``Numbers`` of ``(x, lam)``; ``scale_eps``: the relative deviation of the device's own row scalings (module docstring)."""
        x, lam = np.asarray(x, dtype=np.float64), np.asarray(lam, dtype=np.float64)
        ld = np.longdouble
        yhat, repaired = self.yhat(lam)
        with np.errstate(invalid="ignore", over="ignore"):
            prod = self.vals * yhat[self.rows]                      # rounded products, as the device forms them
            aty = np.zeros(self.N, dtype=ld)
            np.add.at(aty, self.cols, prod.astype(ld))
            mag = np.zeros(self.N)
            np.add.at(mag, self.cols, np.abs(prod))
            d = (self.c.astype(ld) + aty).astype(np.float64)
            e = np.nonzero(self.slack_entry)[0]
            d[self.cols[e]] = prod[e]                               # a slack column: the single double product
            terms = np.where(d != 0, np.minimum(d * self.lb, d * self.ub), 0.0)
            yb = np.where(yhat != 0, yhat * self.b, 0.0)
            cx = self.c * x
            bound = float(np.sum(terms.astype(ld)) - np.sum(yb.astype(ld)))
            primal = float(np.sum(cx.astype(ld)))
            finite = np.isfinite(terms)
            side = np.where(finite, np.maximum(np.abs(np.where(np.isfinite(self.lb), self.lb, 0.0)),
                                               np.abs(np.where(np.isfinite(self.ub), self.ub, 0.0))), 0.0)
            tol_bound = 1.01 * U * ((self.longest_column + 2) * float(np.sum((np.abs(self.c) + mag) * side))
                                    + (self.N + self.m + 2) * float(np.sum(np.abs(terms[finite])) + np.sum(np.abs(yb))))
            tol_primal = 1.01 * U * (self.N + 1) * float(np.sum(np.abs(cx)))
            ax = oracle.matvec(self.a, x)
            violation = float(np.max(np.concatenate((np.abs(ax - self.b), self.lb - x, x - self.ub, [0.0]))))
            tol_violation = float(np.max(oracle.row_error_bound(self.a, x))) if self.m else 0.0
            if scale_eps:
                tol_bound += scale_eps * float(np.sum(mag * side) + np.sum(np.abs(terms[finite])) + np.sum(np.abs(yb)))
                absax = oracle.matvec(oracle.Csr(self.indptr, self.cols, np.abs(self.vals), self.a.shape), np.abs(x))
                box = np.concatenate((self.lb[self.slack], self.ub[self.slack], [0.0]))
                tol_violation += scale_eps * max(float(np.max(absax + np.abs(self.b))) if self.m else 0.0,
                                                 float(np.max(np.abs(box[np.isfinite(box)]))))
        return Numbers(primal, bound, violation, tol_primal, tol_bound, tol_violation, repaired)


def scale_eps(r):
    """``eps = 4 (Lr + 4) u`` of the module docstring for the restatement ``r``."""
    return 4.0 * (r.longest_row + 4) * U


def from_implicit(x, n, m_eq):
    """The iterate of a form with an implicit slack column per row, ``[x_o (n); one slack per row]``, as the standard form of
    ``oracle.admm_setup`` holds it -- the slacks of the equality rows dropped -- and the largest ``|x|`` among those dropped: their
    box is [0, 0], so that is their bound violation."""
    x = np.asarray(x, dtype=np.float64)
    dropped = x[n:n + m_eq]
    return np.concatenate((x[:n], x[n + m_eq:])), (float(np.max(np.abs(dropped))) if dropped.size else 0.0)


def decision(primal, bound, violation, tol_gap, tol_feas):
    """``cp_gap_decide`` from three numbers (scalars)."""
    with np.errstate(invalid="ignore"):
        gap = abs(primal - bound)
        return bool(violation <= tol_feas and np.isfinite(gap) and gap <= tol_gap * (1.0 + abs(primal) + abs(bound)))


def scalar_rule(a, lam, lb, ub):
    """``admm_gap_slack_unbounded`` of csrc/slp_admm_gap.h on scalars: ``(repaired, yhat)``."""
    with np.errstate(invalid="ignore", over="ignore"):
        a, lam, lb, ub = (np.float64(v) for v in (a, lam, lb, ub))
        p = a * lam
        repaired = bool(p != 0.0 and np.minimum(p * lb, p * ub) == -np.inf)
    return repaired, (0.0 if repaired else float(lam))
