"""``SparseLP``: the modelling front end and the ``solve(method=...)`` dispatch.

Keeps the public surface of ``pysparselp.SparseLP.SparseLP`` that the
first-order solvers need (reference SparseLP.py:162-1383): the LP is held as

    minimise costsvector . x
    s.t.     a_equalities x = b_equalities
             b_lower <= a_inequalities x <= b_upper
             lower_bounds <= x <= upper_bounds

with scipy CSR matrices, and ``solve`` (reference :990-1002, :1064-1093,
:1193-1208, :1243-1288, :1378-1383) runs one of the GPU solvers and fills the
same convergence-curve attributes.  The hot-path methods ``"admm"`` and
``"chambolle_pock_ppd"``, the block-splitting ``"admm_blocks"``, ``"admm2"`` (ADMM with exact equality projections) and
``"dual_gradient_ascent"`` (exact line search in the dual) exist here; the other solvers of the reference
(interior point, dual coordinate ascent, external solver bridges, rounding heuristics,
MPS export) are out of scope.
"""
import copy
import time

import numpy as np

import scipy.sparse

from .ADMM import _admm_batch_rhs_run, _check_admm_batch_rhs_call, lp_admm, lp_admm_batch, lp_admm_batch_until
from .ChambollePockPPD import (chambolle_pock_ppd, chambolle_pock_ppd_batch, chambolle_pock_ppd_batch_certified, chambolle_pock_ppd_many,
                               chambolle_pock_ppd_many_certified, chambolle_pock_ppd_many_until)
from ._many import check_stop
from ._batch import check_costs, require_one_sided
from ._lib import ORDER_AUTO

solving_methods = ("chambolle_pock_ppd", "admm", "admm_blocks", "admm2")
# methods that ascend in the dual and return feasible multipliers; ``solve`` accepts ``solving_methods + dual_methods``
dual_methods = ("dual_gradient_ascent",)
# methods of ``solve_batch``: many cost vectors over this LP's constraints, advanced together
batch_methods = ("chambolle_pock_ppd",)
# methods of ``solve_many``: a list of LPs with matrices of their own, one workgroup per LP
many_methods = ("chambolle_pock_ppd",)

_SCALARS = (int, float, np.integer, np.floating)
_CURVES = ("distance_to_ground_truth", "distanceToGroundTruthAfterRounding", "opttime_curve", "dopttime_curve", "pobj_curve",
           "dobj_curve", "pobjbound", "max_violated_inequality", "max_violated_equality", "max_violated_constraint", "itrn_curve")


def _reset_curves(lp):
    for name in _CURVES:
        setattr(lp, name, [])


def _admm_auto_xstep(a_eq, a_ineq):
    """``xstep="auto"`` of ``solve(method="admm")`` and ``solve_admm_certified``: ``"cg"`` when the standard-form rows promise more
    than ``ADMM_AUTO_M_ENTRIES`` entries in ``M`` (sum of squared row lengths) or a communicator is active, else ``"gauss_seidel"``."""
    from .parallel import comm_world

    rows_sq = 0.0
    for blk, slack in ((a_eq, 0), (a_ineq, 1)):
        if blk is not None:
            rows_sq += float(np.sum((np.diff(blk.indptr).astype(np.float64) + slack) ** 2))
    return "cg" if (rows_sq > ADMM_AUTO_M_ENTRIES or comm_world()[0] > 1) else "gauss_seidel"


def _mean_together(distances):
    """Per instance the mean of its distances to the ground truth, one reduction over the whole batch."""
    return np.mean(distances, axis=tuple(range(1, distances.ndim)))


def _mean_each(distances):
    """The same instance by instance: the expressions (and so the sums) of ``solve``."""
    return np.array([np.mean(d) for d in distances])


def _batch_recorder(lp, batch, ground_truth, ground_truth_indices, mean=_mean_together, expand=None, views=None):
    """The callback of the three ``(B, ...)`` forms: fills ``lp``'s curves as ``solve`` does, the per-instance ones with arrays of
    length ``batch`` (a number the solver reports once for all instances is repeated).  ``expand`` maps the solver's iterates to
    the LP's variables.  ``views``: per instance the LP against which its ``max_violated_constraint`` is taken (``_rhs_views``)
    instead of ``lp`` itself."""
    def record(niter, solution, energy1, energy2, duration, max_violated_equality, max_violated_inequality):
        if expand is not None:
            solution = expand(solution)
        if ground_truth is not None:
            picked = solution[:, ground_truth_indices]
            lp.distance_to_ground_truth.append(mean(np.abs(ground_truth - picked)))
            lp.distanceToGroundTruthAfterRounding.append(mean(np.abs(ground_truth - np.round(picked))))
        lp.itrn_curve.append(niter)
        lp.opttime_curve.append(duration)
        lp.dopttime_curve.append(duration)
        lp.dobj_curve.append(np.full(batch, energy2, dtype=np.float64))
        lp.pobj_curve.append(np.full(batch, energy1, dtype=np.float64))
        lp.max_violated_constraint.append(np.array([(lp if views is None else views[k]).max_constraint_violation(solution[k])
                                                    for k in range(batch)]))
        lp.max_violated_equality.append(np.full(batch, max_violated_equality, dtype=np.float64))
        lp.max_violated_inequality.append(np.full(batch, max_violated_inequality, dtype=np.float64))

    return record


def _rhs_views(lp, batch, **sides):
    """Per instance a shallow copy of ``lp`` whose right-hand sides are row k of the given ones (``name=array`` of shape ``(rows,)``
    or ``(batch, rows)``; None keeps the LP's): what instance k's constraint violations are measured against."""
    views = []
    for k in range(batch):
        view = copy.copy(lp)
        for name, v in sides.items():
            if v is not None:
                v = np.asarray(v, dtype=np.float64)
                setattr(view, name, v[k] if v.ndim == 2 else v)
        views.append(view)
    return views


def _list_recorder(lps, expand=None, skip=()):
    """The callback of the two list forms: fills every LP's curves as its own ``solve`` does; a number reported once for the whole
    list goes to every LP as it is.  ``expand(k, x)`` maps the solver's iterate of LP ``k`` to its variables; the LPs with a true
    entry in ``skip`` (filled by the time of the first report) record nothing."""
    def of(number, k):
        return number[k] if np.ndim(number) else number

    def record(niter, solutions, energy1, energy2, duration, max_violated_equality, max_violated_inequality):
        for k, lp in enumerate(lps):
            if k < len(skip) and skip[k]:
                continue
            lp.itrn_curve.append(niter)
            lp.opttime_curve.append(duration)
            lp.dopttime_curve.append(duration)
            lp.dobj_curve.append(of(energy2, k))
            lp.pobj_curve.append(of(energy1, k))
            lp.max_violated_constraint.append(lp.max_constraint_violation(solutions[k] if expand is None else expand(k, solutions[k])))
            lp.max_violated_equality.append(of(max_violated_equality, k))
            lp.max_violated_inequality.append(of(max_violated_inequality, k))

    return record


def empty_csr_matrix(ncols=0):
    a = scipy.sparse.csr_matrix((0, ncols), dtype=np.float64)
    a.__dict__["blocks"] = []
    return a


def _append_rows(a, b):
    """Rows of ``b`` appended under ``a`` (entry order kept); records the row block like the reference."""
    b = scipy.sparse.csr_matrix(b)
    ncols = max(a.shape[1], b.shape[1])
    blocks = a.__dict__.get("blocks", [])
    blocks.append((a.shape[0], a.shape[0] + b.shape[0] - 1))
    out = scipy.sparse.csr_matrix(
        (np.concatenate((a.data, b.data.astype(np.float64))),
         np.concatenate((a.indices, b.indices)).astype(np.int32),
         np.concatenate((a.indptr[:-1], a.indptr[-1] + b.indptr)).astype(np.int32)),
        shape=(a.shape[0] + b.shape[0], ncols))
    out.__dict__["blocks"] = blocks
    return out


def _with_ncols(a, ncols):
    out = scipy.sparse.csr_matrix((a.data, a.indices, a.indptr), shape=(a.shape[0], ncols))
    out.__dict__["blocks"] = a.__dict__.get("blocks", [])
    return out


def crd_matrix(cols, vals):
    """CSR matrix with the same number of candidate entries in every row:
    ``m[i, cols[i, j]] = vals[i, j]``; zero values are not stored; a variable may
    appear only once per row."""
    cols, vals = np.broadcast_arrays(np.asarray(cols), np.asarray(vals, dtype=np.float64))
    assert cols.ndim == 2
    srt = np.sort(cols, axis=1)
    if srt.shape[1] > 1 and np.any(srt[:, 1:] == srt[:, :-1]):
        bad = np.nonzero(np.any(srt[:, 1:] == srt[:, :-1], axis=1))[0]
        raise ValueError(f"the same variable appears twice in {len(bad)} constraint(s): {bad}")
    keep = vals != 0
    indptr = np.concatenate(([0], np.cumsum(keep.sum(axis=1))))
    ncols = int(cols.max()) + 1 if cols.size else 0
    return scipy.sparse.csr_matrix((vals[keep], cols[keep], indptr), shape=(cols.shape[0], ncols))


ADMM_AUTO_M_ENTRIES = 2.0e8  # solve(method="admm", xstep="auto"): above this estimate of nnz(M) the matrix-free x-step is taken
# setup="auto" (solve with "chambolle_pock_ppd" or the matrix-free "admm", chambolle_pock_ppd, lp_admm_cg): from this many stored
# constraint entries on, the LP is set up on the device instead of by the reference's host transforms
DEVICE_SETUP_ENTRIES = 1.0e7


class SparseLP:
    """Sparse linear program + first-order GPU solvers."""

    def __init__(self):
        self.nb_variables = 0
        self.variables_dict = dict()
        self.upper_bounds = np.empty(0, dtype=np.float64)
        self.lower_bounds = np.empty(0, dtype=np.float64)
        self.costsvector = np.empty(0, dtype=np.float64)
        self.is_integer = np.empty(0, dtype=bool)
        self.a_inequalities = empty_csr_matrix()
        self.b_lower = np.empty(0, dtype=np.float64)
        self.b_upper = np.empty(0, dtype=np.float64)
        self.a_equalities = empty_csr_matrix()
        self.b_equalities = np.empty(0, dtype=np.float64)
        self.solution = None

    # ------------------------------------------------------------------ variables
    def _bounds_as_arrays(self, shape, lower_bounds, upper_bounds):
        def expand(v, default):
            if v is None:
                return np.full(shape, default, dtype=np.float64)
            if isinstance(v, _SCALARS):
                return np.full(shape, float(v), dtype=np.float64)
            v = np.asarray(v, dtype=np.float64)
            assert v.shape == tuple(shape)
            return v

        return expand(lower_bounds, -np.inf), expand(upper_bounds, np.inf)

    def add_variables_array(self, shape, lower_bounds, upper_bounds, costs=0, name=None, is_integer=False):
        """Append ``prod(shape)`` variables; returns their indices as an array of that shape."""
        if isinstance(shape, (int, np.integer)):
            shape = (int(shape),)
        shape = tuple(int(s) for s in shape)
        count = int(np.prod(shape))
        indices = np.arange(count).reshape(shape) + self.nb_variables
        self.nb_variables += count
        self.a_inequalities = _with_ncols(self.a_inequalities, self.nb_variables)
        self.a_equalities = _with_ncols(self.a_equalities, self.nb_variables)
        if isinstance(costs, _SCALARS):
            costs = np.full(shape, float(costs))
        costs = np.asarray(costs, dtype=np.float64)
        assert costs.shape == shape
        lo, hi = self._bounds_as_arrays(shape, lower_bounds, upper_bounds)
        self.lower_bounds = np.append(self.lower_bounds, lo.ravel())
        self.upper_bounds = np.append(self.upper_bounds, hi.ravel())
        self.costsvector = np.append(self.costsvector, costs.ravel())
        self.is_integer = np.append(self.is_integer, np.full(count, is_integer, dtype=bool))
        if name:
            self.variables_dict[name] = indices
        return indices

    def get_variables_indices(self, name):
        return self.variables_dict[name]

    def get_variables_bounds(self):
        return None, self.lower_bounds, self.upper_bounds

    def set_costs_variables(self, indices, costs):
        assert np.shape(costs) == np.shape(indices)
        self.costsvector[np.ravel(indices)] = np.ravel(costs)

    def set_bounds_on_variables(self, indices, lower_bounds, upper_bounds):
        lo, hi = self._bounds_as_arrays(np.shape(indices), lower_bounds, upper_bounds)
        self.lower_bounds[np.ravel(indices)] = lo.ravel()
        self.upper_bounds[np.ravel(indices)] = hi.ravel()

    # ---------------------------------------------------------------- constraints
    def nb_equality_constraints(self):
        return self.a_equalities.shape[0]

    def nb_inequality_constraints(self):
        return self.a_inequalities.shape[0]

    def add_equality_constraints_sparse(self, a, b):
        self.a_equalities = _append_rows(self.a_equalities, a)
        self.b_equalities = np.append(self.b_equalities, b)

    def add_inequality_constraints_sparse(self, a, lower_bounds=None, upper_bounds=None):
        """Add ``lower_bounds <= a x <= upper_bounds``; a scalar ``lower == upper`` makes equalities."""
        rows = a.shape[0]
        if isinstance(lower_bounds, (int, float)) and not isinstance(lower_bounds, bool) and lower_bounds == upper_bounds:
            self.a_equalities = _append_rows(self.a_equalities, a)
            self.b_equalities = np.append(self.b_equalities, np.full(rows, float(lower_bounds)))
            return
        lo, hi = self._bounds_as_arrays((rows,), lower_bounds, upper_bounds)
        self.a_inequalities = _append_rows(self.a_inequalities, a)
        self.b_lower = np.append(self.b_lower, lo)
        self.b_upper = np.append(self.b_upper, hi)

    def add_inequality_constraints(self, cols, vals, lower_bounds=None, upper_bounds=None):
        """``lower[i] <= sum_j vals[i, j] x[cols[i, j]] <= upper[i]`` for every row i."""
        self.add_inequality_constraints_sparse(crd_matrix(cols, vals), lower_bounds=lower_bounds, upper_bounds=upper_bounds)

    def add_equality_constraints(self, cols, vals, b):
        self.add_inequality_constraints(cols, vals, lower_bounds=b, upper_bounds=b)

    def add_soft_inequality_constraints(self, cols, vals, coef_penalization, lower_bounds=None, upper_bounds=None):
        """Penalised version: adds ``sum_i coef[i] * max(0, lower[i] - y_i, y_i - upper[i])`` to the objective,
        ``y_i = sum_j vals[i, j] x[cols[i, j]]``, through one auxiliary variable per row (reference :575-613).
        With an infinite penalty this is the hard constraint.  Returns the auxiliary variable indices (or None)."""
        coef = np.asarray(coef_penalization, dtype=np.float64)
        if np.all(coef == np.inf):
            self.add_inequality_constraints(cols, vals, lower_bounds=lower_bounds, upper_bounds=upper_bounds)
            return None
        if np.any(coef == np.inf):
            raise ValueError("mixing finite and infinite penalisation is not supported")
        cols, vals = np.broadcast_arrays(np.asarray(cols), np.asarray(vals, dtype=np.float64))
        assert upper_bounds is not None or lower_bounds is not None
        costs = coef if coef.ndim else float(coef)
        aux = self.add_variables_array((cols.shape[0],), lower_bounds=0, upper_bounds=None, costs=costs)
        cols2 = np.column_stack((cols, aux))
        if upper_bounds is not None:   # y - aux <= upper
            self.add_inequality_constraints(cols2, np.column_stack((vals, -np.ones(vals.shape[0]))), None, upper_bounds)
        if lower_bounds is not None:   # y + aux >= lower
            self.add_inequality_constraints(cols2, np.column_stack((vals, np.ones(vals.shape[0]))), lower_bounds, None)
        return aux

    def add_soft_equality_constraints(self, cols, vals, b, coef_penalization):
        """Adds ``sum_i coef[i] * |y_i - b_i|`` to the objective (reference :546-558)."""
        return self.add_soft_inequality_constraints(cols, vals, coef_penalization, lower_bounds=b, upper_bounds=b)

    # ------------------------------------------------------------------ transforms
    def convert_to_one_sided_inequality_system(self):
        """``b_lower <= A x <= b_upper`` -> ``A' x <= b_upper'`` (finite upper rows, then negated finite lower rows)."""
        if self.a_inequalities is None or self.b_lower is None:
            return
        up = np.nonzero(self.b_upper != np.inf)[0]
        lo = np.nonzero(self.b_lower != -np.inf)[0]
        a = self.a_inequalities
        if len(lo) > 0 and len(up) > 0:
            a = scipy.sparse.vstack((a[up, :], -a[lo, :])).tocsr()
        elif len(lo) > 0:
            a = -a
        a.__dict__["blocks"] = [(0, a.shape[0] - 1)]
        self.a_inequalities = a
        self.b_upper = np.hstack((self.b_upper[up], -self.b_lower[lo]))
        self.b_lower = None

    def remove_fixed_variables(self):
        """Drop the variables with ``upper == lower`` (reference :632-674).

        Returns ``(free, shift)``: the boolean mask of kept variables and the
        vector holding the fixed values; right-hand sides are moved accordingly.
        """
        free = self.upper_bounds > self.lower_bounds
        shift = np.zeros(self.nb_variables)
        shift[~free] = self.lower_bounds[~free]
        self.b_equalities = self.b_equalities - self.a_equalities * shift
        if self.b_lower is not None:
            self.b_lower = self.b_lower - self.a_inequalities * shift
        if self.b_upper is not None:
            self.b_upper = self.b_upper - self.a_inequalities * shift
        for name in ("a_inequalities", "a_equalities"):
            a = getattr(self, name)
            blocks = a.__dict__.get("blocks", [])
            a = a[:, free]
            a.__dict__["blocks"] = blocks
            setattr(self, name, a)
        self.costsvector = self.costsvector[free]
        self.lower_bounds = self.lower_bounds[free]
        self.upper_bounds = self.upper_bounds[free]
        self.nb_variables = int(np.sum(free))
        return free, shift

    # ---------------------------------------------------------------------- checks
    def max_constraint_violation(self, solution):
        """Largest violation of any bound or constraint of the (unscaled) LP (reference :186-204)."""
        worst = 0
        worst = max(worst, np.max(self.lower_bounds - solution))
        worst = max(worst, np.max(solution - self.upper_bounds))
        if self.a_equalities.shape[0] > 0:
            worst = max(worst, np.max(np.abs(self.a_equalities * solution - self.b_equalities)))
        if self.a_inequalities.shape[0] > 0:
            ax = self.a_inequalities * solution
            if self.b_upper is not None:
                worst = max(worst, np.max(ax - self.b_upper))
            if self.b_lower is not None:
                worst = max(worst, np.max(self.b_lower - ax))
        return worst

    def check_solution(self, solution, tol=1e-6):
        return bool(self.max_constraint_violation(solution) < tol)

    # ------------------------------------------------------------------------- I/O
    def save_mps(self, filename, exact=True):
        """Write the LP as an MPS file (reference SparseLP.py:280-366: objective row ``OBJ``, equality rows ``E<i>``,
        inequality rows ``I<i>``, variables ``X<j>``, right-hand-side set ``RHS0``, bound set ``bound``).

        Differences from the reference, which cannot run as written (``a_eq.ruse_preconditioning``, :310) and prints six
        decimals: numbers are written with 17 significant digits, so that reading the file back
        (``MPSparser.mps_parser``) returns the arrays bit for bit; two-sided and lower-bounded inequality rows are written
        (``G`` rows, ``RANGES`` -- the reference asserts ``b_lower is None``); bounds are written only where they differ
        from the MPS default ``[0, +inf)``.  Integer variables are refused (the reader refuses them too).  A two-sided row
        whose bounds neither ``rhs - range`` nor ``rhs + range`` reproduces in fp64 raises ``ValueError`` (``exact=False``:
        written in the L form, its lower bound then comes back within one ulp)."""
        if np.any(self.is_integer):
            raise NotImplementedError("save_mps: integer variables are not supported")
        n = self.nb_variables
        a_eq, a_in = scipy.sparse.csc_matrix(self.a_equalities), scipy.sparse.csc_matrix(self.a_inequalities)
        m_in = a_in.shape[0]
        up = np.full(m_in, np.inf) if self.b_upper is None else np.asarray(self.b_upper, dtype=np.float64)
        lo = np.full(m_in, -np.inf) if self.b_lower is None else np.asarray(self.b_lower, dtype=np.float64)
        if np.any(np.isneginf(lo) & np.isposinf(up)):
            raise ValueError("save_mps: an inequality row without any finite bound cannot be written")

        def num(v):
            return "%.17g" % v

        with open(filename, "w") as f:
            f.write("NAME          exportedFromPython\nROWS\n N  OBJ\n")
            for i in range(a_eq.shape[0]):
                f.write(" E  E%d\n" % i)
            # a two-sided row is an L row with a range (b_lower = rhs - range) unless only the G form (b_upper = rhs + range)
            # reproduces both bounds exactly
            g_row = ~np.isfinite(up)
            both = np.isfinite(up) & np.isfinite(lo)
            with np.errstate(invalid="ignore"):
                l_exact, g_exact = up - (up - lo) == lo, lo + (up - lo) == up
            g_row |= both & ~l_exact & g_exact
            if exact and np.any(both & ~l_exact & ~g_exact):
                # neither rhs - range nor rhs + range gives the other bound back in fp64: the file could not return the arrays bit
                # for bit (the promise above), so refuse instead of writing a bound that is off by an ulp
                bad = int(np.nonzero(both & ~l_exact & ~g_exact)[0][0])
                raise ValueError("save_mps: the two bounds of inequality row %d cannot be written exactly as a right-hand side and a "
                                 "range; split it into an upper-bounded and a lower-bounded row, or pass exact=False" % bad)
            for i in range(m_in):
                f.write(" %s  I%d\n" % ("G" if g_row[i] else "L", i))
            f.write("COLUMNS\n")
            for j in range(n):
                f.write("    X%-9d OBJ        %s\n" % (j, num(self.costsvector[j])))
                for k in range(a_eq.indptr[j], a_eq.indptr[j + 1]):
                    f.write("    X%-9d E%-9d %s\n" % (j, a_eq.indices[k], num(a_eq.data[k])))
                for k in range(a_in.indptr[j], a_in.indptr[j + 1]):
                    f.write("    X%-9d I%-9d %s\n" % (j, a_in.indices[k], num(a_in.data[k])))
            f.write("RHS\n")
            for i in range(a_eq.shape[0]):
                f.write("    RHS0       E%-9d %s\n" % (i, num(self.b_equalities[i])))
            for i in range(m_in):
                f.write("    RHS0       I%-9d %s\n" % (i, num(lo[i] if g_row[i] else up[i])))
            f.write("RANGES\n")
            for i in range(m_in):
                if np.isfinite(up[i]) and np.isfinite(lo[i]):
                    f.write("    RNG0       I%-9d %s\n" % (i, num(up[i] - lo[i])))
            f.write("BOUNDS\n")
            for j in range(n):
                l, u = self.lower_bounds[j], self.upper_bounds[j]
                if np.isneginf(l) and np.isposinf(u):
                    f.write(" FR bound      X%d\n" % j)
                    continue
                if l == u:
                    f.write(" FX bound      X%-9d %s\n" % (j, num(l)))
                    continue
                if np.isneginf(l):
                    f.write(" MI bound      X%d\n" % j)
                elif l != 0:
                    f.write(" LO bound      X%-9d %s\n" % (j, num(l)))
                if not np.isposinf(u):
                    f.write(" UP bound      X%-9d %s\n" % (j, num(u)))
            f.write("ENDATA\n")

    # ----------------------------------------------------------------------- solve
    def solve(
        self,
        method="admm",
        get_timing=True,
        x0=None,
        nb_iter=10000,
        max_time=None,
        callback_func=None,
        nb_iter_plot=10,
        plot_solution=None,
        ground_truth=None,
        ground_truth_indices=None,
        order=ORDER_AUTO,
        xstep="gauss_seidel",
        setup="auto",
    ):
        """Run a first-order solver on the GPU; returns ``(x, elapsed)`` or ``x``.

        Extensions (keyword-only in spirit; the reference's positional arguments are unchanged): ``order`` -- summation
        order of the dot products (include/slp_hip.h); ``xstep`` for ``method="admm"`` -- ``"gauss_seidel"`` is the
        reference as shipped (one projected Gauss-Seidel sweep on the explicit ``M = 2 A^T A + 3 I``, ADMM.py:162),
        ``"cg"`` its conjugate-gradient branch (ADMM.py:182-201) run matrix-free -- the ADMM that exists where ``M`` cannot
        (1000 entries per row: ``M`` is dense) and the one that shards over several GPUs -- and ``"auto"`` picks ``"cg"``
        when the standard-form rows promise more than ``ADMM_AUTO_M_ENTRIES`` (2e8) entries in ``M`` (sum of squared row
        lengths) or a communicator is active (the sequential sweep does not partition), else ``"gauss_seidel"``.

        ``setup`` (extension) for ``"chambolle_pock_ppd"`` and the matrix-free ``"admm"``: ``"host"`` prepares the solver as the
        reference does (for Chambolle-Pock: ``copy.deepcopy`` and ``remove_fixed_variables`` on the host, then the one-sided
        stacking, SparseLP.py:1244-1248), ``"device"`` uploads the constraint blocks as they are and does all of it on the device,
        ``"auto"`` takes the device from ``DEVICE_SETUP_ENTRIES`` (1e7) stored entries on.  Same ``x`` and curves either way.

        Under a communicator (``parallel.init_comm_from_env`` in every rank of a ``torch.distributed.run`` / ``mpirun``
        launch) every rank calls ``solve`` on the same LP: ``"chambolle_pock_ppd"`` and ``"admm"`` with ``xstep="cg"`` hand
        over only this rank's block of constraint rows (equal stored entries per rank), exchange one / two all-reduces of
        the variable vector per iteration and return the same ``x`` on every rank; the exact Gauss-Seidel ADMM,
        ``admm_blocks`` and ``admm2`` run as replicas.

        ``"admm2"`` is the reference's ``lp_admm2`` (ADMM.py:272-474) with its KKT solves matrix-free (conjugate gradients on
        the device, see ``ADMM.lp_admm2``); ``setup`` and ``order`` do not apply to it.

        ``"dual_gradient_ascent"`` (one of ``dual_methods``) is the reference's method of that name (SparseLP.py:1290-1300,
        ``DualGradientAscent.dual_gradient_ascent``): it reports every 100 iterations whatever ``nb_iter_plot``, refuses a finite
        ``b_lower`` with ``ValueError``, and runs as a replica under a communicator; ``setup`` and ``order`` do not apply.

        Fills, at every report (every ``nb_iter_plot`` iterations): ``itrn_curve,
        opttime_curve, dopttime_curve, pobj_curve, dobj_curve,
        max_violated_constraint, max_violated_equality, max_violated_inequality,
        distance_to_ground_truth, distanceToGroundTruthAfterRounding``.
        As in the reference, ``callback_func`` is accepted and unused (it is
        shadowed by the internal bookkeeping callback, reference :997,:1064).
        """
        if method not in solving_methods + dual_methods:
            raise ValueError(f"method {method!r} not valid; available methods: {solving_methods + dual_methods}")
        if method == "dual_gradient_ascent" and self.b_lower is not None and np.size(self.b_lower) and np.max(self.b_lower) != -np.inf:
            raise ValueError("dual_gradient_ascent needs one-sided inequalities: b_lower must be None or all -inf")
        a_ineq = self.a_inequalities if (self.a_inequalities is not None and self.a_inequalities.shape[0] > 0) else None
        a_eq, b_eq = (self.a_equalities, self.b_equalities) if self.a_equalities.shape[0] > 0 else (None, None)
        if a_ineq is not None:
            assert a_ineq.indices.size == 0 or a_ineq.indices.max() < a_ineq.shape[1]
        start = time.perf_counter()
        _reset_curves(self)
        record = self._curve_recorder(ground_truth, ground_truth_indices, plot_solution)

        if method == "admm":
            if xstep == "auto":
                xstep = _admm_auto_xstep(a_eq, a_ineq)
            x = lp_admm(self.costsvector, a_eq, b_eq, a_ineq, self.b_lower, self.b_upper, self.lower_bounds,
                        self.upper_bounds, nb_iter=nb_iter, x0=x0, callback_func=record, max_time=max_time,
                        nb_iter_plot=nb_iter_plot, order=order, xstep=xstep, setup=setup)
        elif method == "admm_blocks":  # reference :1210-1225
            from .ADMMBlocks import lp_admm_block_decomposition

            x = lp_admm_block_decomposition(self.costsvector, a_eq, b_eq, a_ineq, self.b_lower, self.b_upper, self.lower_bounds,
                                            self.upper_bounds, nb_iter=nb_iter, nb_iter_plot=nb_iter_plot, x0=x0,
                                            callback_func=record, max_time=max_time)
        elif method == "admm2":  # reference :1226-1241: no deep copy, no fixed-variable removal
            from .ADMM import lp_admm2

            x = lp_admm2(self.costsvector, a_eq, b_eq, a_ineq, self.b_lower, self.b_upper, self.lower_bounds, self.upper_bounds,
                         nb_iter=nb_iter, x0=x0, callback_func=record, max_time=max_time, nb_iter_plot=nb_iter_plot)
        elif method == "dual_gradient_ascent":  # reference :1290-1300
            from .DualGradientAscent import dual_gradient_ascent

            x, _, _ = dual_gradient_ascent(x=x0, lp=self, nb_max_iter=nb_iter, callback_func=record, y_eq=None, y_ineq=None,
                                           max_time=max_time, nb_iter_plot=nb_iter_plot)
        else:  # chambolle_pock_ppd: fixed variables are eliminated first (reference :1244-1248)
            x, _ = self._solve_cp(a_eq, b_eq, a_ineq, record, start, nb_iter, max_time, nb_iter_plot, order, setup)
        elapsed = time.perf_counter() - start
        return (x, elapsed) if get_timing else x

    def _curve_recorder(self, ground_truth, ground_truth_indices, plot_solution=None):
        """The callback that fills the curve attributes of ``solve`` at every report."""
        def record(niter, solution, energy1, energy2, duration, max_violated_equality, max_violated_inequality):
            if ground_truth is not None:
                picked = solution[ground_truth_indices]
                self.distance_to_ground_truth.append(np.mean(np.abs(ground_truth - picked)))
                self.distanceToGroundTruthAfterRounding.append(np.mean(np.abs(ground_truth - np.round(picked))))
            self.itrn_curve.append(niter)
            self.opttime_curve.append(duration)
            self.dopttime_curve.append(duration)
            self.dobj_curve.append(energy2)
            self.pobj_curve.append(energy1)
            self.max_violated_constraint.append(self.max_constraint_violation(solution))
            self.max_violated_equality.append(max_violated_equality)
            self.max_violated_inequality.append(max_violated_inequality)
            if plot_solution is not None:
                plot_solution(niter, solution, is_active_variable=None)

        return record

    def _solve_cp(self, a_eq, b_eq, a_ineq, record, start, nb_iter, max_time, nb_iter_plot, order, setup, gap=None):
        """The Chambolle-Pock branch of ``solve`` (``gap`` None) and of ``solve_certified`` (``gap`` the checked ``(tol_gap, tol_feas,
        check_every)``): the reduction, the solver and ``expand``.  Returns ``(x, info)``, ``info`` None without a test."""
        from . import host_setup
        from .ChambollePockPPD import _cp_loop, _gap_info, chambolle_pock_ppd_certified, close_device_cp, device_cp

        device = (a_eq is not None or a_ineq is not None) and host_setup.choose(setup, host_setup.nnz_of(a_eq, a_ineq)) == "device"
        if device:  # no deep copy, no host remove_fixed_variables: the fixed variables are dropped on the device
            state, free, shift = device_cp(self.costsvector, a_eq, b_eq, a_ineq, self.b_lower, self.b_upper, self.lower_bounds,
                                           self.upper_bounds, x0=None, alpha=1, theta=1, order=order, remove_fixed=True)
        else:
            reduced = copy.deepcopy(self)
            free, shift = reduced.remove_fixed_variables()
        free_ids = np.nonzero(free)[0]

        def expand(sol):
            # reference :1259,:1288: x = m_change * sol - shift (note the sign it applies to the fixed values)
            full = np.zeros(free.size)
            full[free_ids] = sol
            return full - shift

        def record_reduced(niter, solution, *rest):
            record(niter, expand(solution), *rest)

        info = None
        if device:
            # (the iterate over the free variables goes through expand: DeviceCP.x() puts the fixed ones at +shift)
            try:
                if gap is not None:
                    state.set_stop_gap(*gap)
                x, _ = _cp_loop(state, self.costsvector[free], state.n, a_ineq is not None, nb_iter, nb_iter_plot, record_reduced,
                                max_time, start, lambda st: st.x_reduced(), None if gap is None else lambda: state.gap_state()[1])
                if gap is not None:
                    info = _gap_info(state)
            finally:
                close_device_cp(state)
        elif gap is not None:
            x, _, info = chambolle_pock_ppd_certified(reduced.costsvector, reduced.a_equalities, reduced.b_equalities,
                                                      reduced.a_inequalities, reduced.b_lower, reduced.b_upper, reduced.lower_bounds,
                                                      reduced.upper_bounds, *gap, x0=None, alpha=1, theta=1, nb_max_iter=nb_iter,
                                                      callback_func=record_reduced, max_time=max_time, nb_iter_plot=nb_iter_plot,
                                                      order=order, setup="host")
        else:
            x, _ = chambolle_pock_ppd(reduced.costsvector, reduced.a_equalities, reduced.b_equalities,
                                      reduced.a_inequalities, reduced.b_lower, reduced.b_upper, reduced.lower_bounds,
                                      reduced.upper_bounds, x0=None, alpha=1, theta=1, nb_max_iter=nb_iter,
                                      callback_func=record_reduced, max_time=max_time, nb_iter_plot=nb_iter_plot,
                                      order=order, setup="host")
        return expand(x), info

    def solve_certified(
        self,
        tol_gap,
        tol_feas,
        check_every=10,
        get_timing=True,
        nb_iter=10000,
        max_time=None,
        nb_iter_plot=10,
        ground_truth=None,
        ground_truth_indices=None,
        order=ORDER_AUTO,
        setup="auto",
    ):
        """``solve(method="chambolle_pock_ppd")`` with a certificate as the stopping test
        (``ChambollePockPPD.chambolle_pock_ppd_certified``): it stops at the first iteration ``t`` with ``t % check_every == 0`` at
        which the violation of the iterate is at most ``tol_feas`` and the gap between its primal value and a valid lower bound is
        at most ``tol_gap * (1 + |primal| + |bound|)``, or after ``nb_iter`` iterations.  Returns ``(x, elapsed)`` or ``x``;
        ``tol_gap`` and ``tol_feas`` finite floats ``>= 0`` and ``check_every`` an int ``>= 1``, a ``ValueError`` otherwise.

        The reduction (``remove_fixed_variables``, on the host or on the device by ``setup``), the curves and the row partition
        under a communicator are those of ``solve``; the loop ends, without a report, at the first report that finds the solver
        stopped.  ``x`` is bit for bit ``solve("chambolle_pock_ppd", nb_iter=stop_info["iterations"])``.

        Sets ``self.stop_info``: ``iterations`` (whole iterations completed), ``stopped``, and the last evaluated certificate
        ``primal``, ``lower_bound``, ``violation``.  These three are the numbers of the LP the solver holds, AFTER
        ``remove_fixed_variables``: the cost of the removed variables at their fixed values is not in them.  It is given separately
        as ``fixed_cost``; add it to ``primal`` and to ``lower_bound`` for the value and the bound of the LP as it was handed in.
        """
        from ._cp_gap import check_gap

        gap = check_gap(tol_gap, tol_feas, check_every)
        a_ineq = self.a_inequalities if (self.a_inequalities is not None and self.a_inequalities.shape[0] > 0) else None
        a_eq, b_eq = (self.a_equalities, self.b_equalities) if self.a_equalities.shape[0] > 0 else (None, None)
        start = time.perf_counter()
        _reset_curves(self)
        record = self._curve_recorder(ground_truth, ground_truth_indices)
        x, info = self._solve_cp(a_eq, b_eq, a_ineq, record, start, nb_iter, max_time, nb_iter_plot, order, setup, gap)
        fixed = ~(self.upper_bounds > self.lower_bounds)
        self.stop_info = dict(info, fixed_cost=float(np.dot(self.costsvector[fixed], self.lower_bounds[fixed])))
        elapsed = time.perf_counter() - start
        return (x, elapsed) if get_timing else x

    def solve_admm_certified(
        self,
        tol_gap,
        tol_feas,
        check_every=10,
        xstep="gauss_seidel",
        get_timing=True,
        x0=None,
        nb_iter=10000,
        max_time=None,
        nb_iter_plot=10,
        ground_truth=None,
        ground_truth_indices=None,
        order=ORDER_AUTO,
        setup="auto",
    ):
        """``solve(method="admm")`` with a certificate as the stopping test (``ADMM.lp_admm_certified``): it stops at the first
        iteration ``t`` with ``t % check_every == 0`` at which the violation of the iterate is at most ``tol_feas`` and the gap
        between its primal value and a valid lower bound is at most ``tol_gap * (1 + |primal| + |bound|)``, or after the
        ``nb_iter + 1`` iterations of ``solve``.  Returns ``(x, elapsed)`` or ``x``; ``tol_gap`` and ``tol_feas`` finite floats
        ``>= 0`` and ``check_every`` an int ``>= 1``, a ``ValueError`` otherwise, before any library is touched.

        ``xstep`` is ``"gauss_seidel"``, ``"cg"`` or ``"auto"`` as in ``solve``, and so are ``setup``, the curves and the row
        partition of ``"cg"`` under a communicator; the loop ends, without a report, at the first report that finds the solver
        stopped.  ``x`` is bit for bit ``solve("admm", nb_iter=stop_info["iterations"] - 1, xstep=...)``.

        Sets ``self.stop_info``, with the keys of ``solve_certified``: ``iterations`` (whole iterations completed), ``stopped``,
        and the last evaluated certificate ``primal``, ``lower_bound``, ``violation``.  These three are the numbers of the
        standard form the solver holds; its value is the LP's, but ``violation`` is in the solver's row-normalised units, not
        in those of ``max_constraint_violation``.  ADMM runs no ``remove_fixed_variables``, so ``fixed_cost`` is 0.0: nothing is
        to be added to ``primal`` or ``lower_bound``."""
        from ._cp_gap import check_gap
        from .ADMM import lp_admm_certified

        gap = check_gap(tol_gap, tol_feas, check_every)
        if xstep not in ("gauss_seidel", "cg", "auto"):
            raise ValueError(f"unknown xstep {xstep!r}: 'gauss_seidel', 'cg' or 'auto'")
        a_ineq = self.a_inequalities if (self.a_inequalities is not None and self.a_inequalities.shape[0] > 0) else None
        a_eq, b_eq = (self.a_equalities, self.b_equalities) if self.a_equalities.shape[0] > 0 else (None, None)
        start = time.perf_counter()
        _reset_curves(self)
        record = self._curve_recorder(ground_truth, ground_truth_indices)
        if xstep == "auto":
            xstep = _admm_auto_xstep(a_eq, a_ineq)
        x, info = lp_admm_certified(self.costsvector, a_eq, b_eq, a_ineq, self.b_lower, self.b_upper, self.lower_bounds,
                                    self.upper_bounds, *gap, x0=x0, nb_iter=nb_iter, callback_func=record, max_time=max_time,
                                    nb_iter_plot=nb_iter_plot, order=order, xstep=xstep, setup=setup)
        self.stop_info = dict(info, fixed_cost=0.0)
        elapsed = time.perf_counter() - start
        return (x, elapsed) if get_timing else x

    def solve_batch(
        self,
        costs,
        method="chambolle_pock_ppd",
        get_timing=True,
        nb_iter=10000,
        max_time=None,
        nb_iter_plot=10,
        ground_truth=None,
        ground_truth_indices=None,
    ):
        """Solve this LP once for every row of ``costs`` (shape ``(B, nb_variables)``) in place of ``costsvector``, all B solves
        advancing together on the GPU (extension: the reference solves one LP per call); returns ``(X, elapsed)`` or ``X``,
        ``X`` of shape ``(B, nb_variables)``.

        Only ``method="chambolle_pock_ppd"`` exists in batched form (``ChambollePockPPD.chambolle_pock_ppd_batch``); any other
        raises ``ValueError``.  Bounds and right-hand sides are the LP's own, so ``remove_fixed_variables`` is one reduction for
        all instances, done once on the host as ``solve(setup="host")`` does (reference :1244-1248); ``X[k]`` and the k-th
        component of every curve are what ``solve(method="chambolle_pock_ppd", order=ORDER_SEQUENTIAL)`` gives on a copy of the LP
        whose ``costsvector`` is ``costs[k]`` (``x`` bit for bit).

        Fills the curve attributes of ``solve`` at every report: ``itrn_curve``, ``opttime_curve``, ``dopttime_curve`` are lists of
        scalars; ``pobj_curve``, ``dobj_curve``, ``max_violated_equality``, ``max_violated_inequality``, ``max_violated_constraint``
        (and, with ``ground_truth``, the two distance curves) are lists of arrays of length B.  ``max_time`` stops the whole
        batch.  Under a communicator every rank solves the whole batch (a replica).
        """
        if method not in batch_methods:
            raise ValueError(f"method {method!r} has no batched form; solve_batch supports: {batch_methods}")
        costs, batch = check_costs(costs, self.nb_variables)
        start = time.perf_counter()
        _reset_curves(self)
        reduced = copy.deepcopy(self)
        free, shift = reduced.remove_fixed_variables()
        free_ids = np.nonzero(free)[0]

        def expand(sol):
            # reference :1259,:1288 per instance: x = m_change * sol - shift (note the sign it applies to the fixed values)
            full = np.zeros((sol.shape[0], free.size))
            full[:, free_ids] = sol
            return full - shift

        record = _batch_recorder(self, batch, ground_truth, ground_truth_indices, expand=expand)
        res = chambolle_pock_ppd_batch(costs[:, free], reduced.a_equalities, reduced.b_equalities, reduced.a_inequalities,
                                       reduced.b_lower, reduced.b_upper, reduced.lower_bounds, reduced.upper_bounds, x0=None, alpha=1,
                                       theta=1, nb_max_iter=nb_iter, callback_func=record, max_time=max_time, nb_iter_plot=nb_iter_plot)
        x = expand(res[0] if isinstance(res, tuple) else res)
        elapsed = time.perf_counter() - start
        return (x, elapsed) if get_timing else x

    def solve_batch_certified(
        self,
        costs,
        tol_gap,
        tol_feas,
        check_every=10,
        get_timing=True,
        nb_iter=10000,
        max_time=None,
        nb_iter_plot=10,
        ground_truth=None,
        ground_truth_indices=None,
    ):
        """``solve_batch`` with a certificate as the stopping test per instance
        (``ChambollePockPPD.chambolle_pock_ppd_batch_certified``): every instance stops on its own at the first iteration ``t`` with
        ``t % check_every == 0`` at which its violation is at most ``tol_feas`` and the gap between its primal value and a valid
        lower bound is at most ``tol_gap * (1 + |primal| + |bound|)``; the others go on, at most ``nb_iter`` iterations.  Returns
        ``(X, elapsed)`` or ``X``; ``tol_gap`` and ``tol_feas`` finite floats ``>= 0`` and ``check_every`` an int ``>= 1``, a
        ``ValueError`` otherwise.

        The reduction (``remove_fixed_variables``, once for all instances) and the curves are those of ``solve_batch``; the loop
        ends at the first report at which every instance is stopped, and a stopped instance's curve entries repeat its last
        running row.  ``X[k]`` is bit for bit ``solve_batch(costs, nb_iter=batch_info["iterations"][k])[k]``.

        Sets ``self.batch_info``, a dict of arrays of length B: ``iterations`` (completed; for a stopped instance its stopping
        iteration), ``stopped``, and the last evaluated certificate ``primal``, ``lower_bound``, ``violation``.  These three are
        the numbers of the LP the solver holds, AFTER ``remove_fixed_variables``: the cost of the removed variables at their
        fixed values is not in them.  It is given separately as ``fixed_cost`` (per instance, from its row of ``costs``); add it
        to ``primal`` and to ``lower_bound`` for the value and the bound of the LP as it was handed in.
        """
        check_stop(tol_gap, check_every, "tol_gap")
        check_stop(tol_feas, check_every, "tol_feas")
        costs, batch = check_costs(costs, self.nb_variables)
        start = time.perf_counter()
        _reset_curves(self)
        reduced = copy.deepcopy(self)
        free, shift = reduced.remove_fixed_variables()
        free_ids = np.nonzero(free)[0]

        def expand(sol):
            # reference :1259,:1288 per instance: x = m_change * sol - shift (note the sign it applies to the fixed values)
            full = np.zeros((sol.shape[0], free.size))
            full[:, free_ids] = sol
            return full - shift

        record = _batch_recorder(self, batch, ground_truth, ground_truth_indices, expand=expand)
        sol, _, info = chambolle_pock_ppd_batch_certified(
            costs[:, free], reduced.a_equalities, reduced.b_equalities, reduced.a_inequalities, reduced.b_lower, reduced.b_upper,
            reduced.lower_bounds, reduced.upper_bounds, tol_gap, tol_feas, check_every, x0=None, alpha=1, theta=1, nb_max_iter=nb_iter,
            callback_func=record, max_time=max_time, nb_iter_plot=nb_iter_plot)
        x = expand(sol)
        fixed = ~(self.upper_bounds > self.lower_bounds)
        self.batch_info = dict(info, fixed_cost=costs[:, fixed].dot(self.lower_bounds[fixed]))
        elapsed = time.perf_counter() - start
        return (x, elapsed) if get_timing else x

    def solve_admm_batch(
        self,
        costs,
        get_timing=True,
        nb_iter=10000,
        max_time=None,
        nb_iter_plot=10,
        ground_truth=None,
        ground_truth_indices=None,
    ):
        """Solve this LP with ``method="admm"`` once for every row of ``costs`` (shape ``(B, nb_variables)``) in place of
        ``costsvector``, all B solves advancing together on the GPU (``ADMM.lp_admm_batch``; extension: the reference solves one LP
        per call); returns ``(X, elapsed)`` or ``X``, ``X`` of shape ``(B, nb_variables)``.

        Bounds, constraints and right-hand sides are the LP's own.  ``X[k]`` and the k-th component of every curve are what
        ``solve(method="admm", order=ORDER_SEQUENTIAL, setup="host")`` gives on a copy of the LP whose ``costsvector`` is
        ``costs[k]`` (``x`` and the violation curves bit for bit, the energies to the rounding of another summation order).
        ``solve_batch(method="admm")`` keeps refusing: the batched Chambolle-Pock and this method fill their curves alike but
        report at different places of their iterations.

        Fills the curve attributes of ``solve`` at every report: ``itrn_curve``, ``opttime_curve``, ``dopttime_curve`` are lists of
        scalars; ``pobj_curve``, ``dobj_curve``, ``max_violated_equality``, ``max_violated_inequality``, ``max_violated_constraint``
        (and, with ``ground_truth``, the two distance curves) are lists of arrays of length B.  ``max_time`` stops the whole
        batch.  Under a communicator every rank solves the whole batch (a replica).
        """
        out = self._solve_admm_batch(costs, None, get_timing, nb_iter, max_time, nb_iter_plot, ground_truth, ground_truth_indices)
        return out[:2] if get_timing else out[0]

    def _solve_admm_batch(self, costs, stop, get_timing, nb_iter, max_time, nb_iter_plot, ground_truth, ground_truth_indices):
        """``solve_admm_batch`` (``stop`` None) and ``solve_admm_batch_until`` (``stop`` its ``(tol_residual, tol_step,
        check_every)``): what ``solve_admm_batch`` returns as a tuple, with ``info`` (None without a test) appended."""
        costs, batch = check_costs(costs, self.nb_variables)
        a_ineq = self.a_inequalities if (self.a_inequalities is not None and self.a_inequalities.shape[0] > 0) else None
        a_eq, b_eq = (self.a_equalities, self.b_equalities) if self.a_equalities.shape[0] > 0 else (None, None)
        start = time.perf_counter()
        _reset_curves(self)

        record = _batch_recorder(self, batch, ground_truth, ground_truth_indices)
        args = (costs, a_eq, b_eq, a_ineq, self.b_lower, self.b_upper, self.lower_bounds, self.upper_bounds)
        kw = dict(nb_iter=nb_iter, callback_func=record, max_time=max_time, nb_iter_plot=nb_iter_plot)
        x, info = (lp_admm_batch(*args, **kw), None) if stop is None else lp_admm_batch_until(*args, *stop, **kw)
        elapsed = time.perf_counter() - start
        return (x, elapsed, info) if get_timing else (x, info)

    def solve_admm_batch_until(
        self,
        costs,
        tol_residual,
        tol_step,
        check_every=10,
        get_timing=True,
        nb_iter=10000,
        max_time=None,
        nb_iter_plot=10,
        ground_truth=None,
        ground_truth_indices=None,
    ):
        """``solve_admm_batch`` with a stopping test per instance (``ADMM.lp_admm_batch_until``): every instance stops on its own at
        the first iteration ``t`` with ``t % check_every == 0`` at which ``max|A x_t - b| <= tol_residual`` and
        ``max|x_t - x_{t-1}| <= tol_step`` (standard form, slacks included); the others go on, at most ``nb_iter + 1`` sweeps.
        Returns ``(X, elapsed, info)`` or ``(X, info)``: what ``solve_admm_batch`` returns, plus ``info``, the dict of arrays of
        length B of ``lp_admm_batch_until`` (``iterations``, ``stopped``, ``residual``, ``step``).  ``tol_residual`` and ``tol_step``
        finite floats ``>= 0`` and ``check_every`` an int ``>= 1``, a ``ValueError`` that names the argument otherwise.

        The LP is handed over as ``solve_admm_batch`` hands it over (no variable is removed) and the curves are filled alike, one
        entry per report; the loop ends at the first report index at which every instance is stopped.  A stopped instance's entries
        are the report on its final iterate.
        """
        check_stop(tol_residual, check_every, "tol_residual")
        check_stop(tol_step, check_every, "tol_step")
        return self._solve_admm_batch(costs, (tol_residual, tol_step, check_every), get_timing, nb_iter, max_time, nb_iter_plot,
                                      ground_truth, ground_truth_indices)

    def solve_admm_batch_rhs(
        self,
        costs,
        b_equalities=None,
        b_lower=None,
        b_upper=None,
        tol_residual=None,
        tol_step=None,
        check_every=10,
        get_timing=True,
        nb_iter=10000,
        max_time=None,
        nb_iter_plot=10,
        ground_truth=None,
        ground_truth_indices=None,
    ):
        """``solve_admm_batch`` / ``solve_admm_batch_until`` with right-hand sides per instance (``ADMM.lp_admm_batch_rhs``):
        ``b_equalities`` of shape ``(m_eq,)`` or ``(B, m_eq)``, ``b_lower`` and ``b_upper`` ``(m_ineq,)`` or ``(B, m_ineq)``, each
        defaulting to the LP's own.  Returns what ``solve_admm_batch_until`` returns, ``(X, elapsed, info)`` or ``(X, info)``;
        ``info`` is None without ``tol_residual`` / ``tol_step`` (optional, both or neither).

        ``X[k]`` and the k-th component of every curve are what ``solve(method="admm", order=ORDER_SEQUENTIAL, setup="host")``
        gives on a copy of the LP whose ``costsvector`` is ``costs[k]`` and whose right-hand sides are row k; ``max_violated_*`` of
        instance k is taken against instance k's right-hand sides.  The curves are filled as by ``solve_admm_batch``."""
        costs, batch = check_costs(costs, self.nb_variables)
        a_ineq = self.a_inequalities if (self.a_inequalities is not None and self.a_inequalities.shape[0] > 0) else None
        a_eq = self.a_equalities if self.a_equalities.shape[0] > 0 else None
        b_eq = None if a_eq is None else (self.b_equalities if b_equalities is None else b_equalities)
        b_lower = self.b_lower if b_lower is None else b_lower
        b_upper = self.b_upper if b_upper is None else b_upper
        # the checks of lp_admm_batch_rhs, made once and before the curves are touched
        stop, rhs = _check_admm_batch_rhs_call(costs, a_eq, b_eq, a_ineq, b_lower, b_upper, tol_residual, tol_step, check_every)
        start = time.perf_counter()
        _reset_curves(self)
        views = _rhs_views(self, batch, b_equalities=rhs[0], b_lower=rhs[1], b_upper=rhs[2])
        record = _batch_recorder(self, batch, ground_truth, ground_truth_indices, views=views)
        x, info = _admm_batch_rhs_run(costs, a_eq, b_eq, a_ineq, rhs, self.lower_bounds, self.upper_bounds, stop, None, 2, 3, nb_iter, record,
                                      max_time, True, nb_iter_plot)
        elapsed = time.perf_counter() - start
        return (x, elapsed, info) if get_timing else (x, info)

    def solve_dga_batch_rhs(
        self,
        costs,
        b_equalities=None,
        b_upper=None,
        tol=None,
        targets=None,
        check_every=10,
        get_timing=True,
        nb_iter=10000,
        max_time=None,
        nb_iter_plot=10,
        ground_truth=None,
        ground_truth_indices=None,
        lower_bounds=None,
        upper_bounds=None,
    ):
        """``solve_dga_batch`` / ``solve_dga_batch_until`` with right-hand sides per instance
        (``DualGradientAscent.dual_gradient_ascent_batch_rhs``): ``b_equalities`` of shape ``(m_eq,)`` or ``(B, m_eq)``, ``b_upper``
        ``(m_ineq,)`` or ``(B, m_ineq)``, each defaulting to the LP's own.  Returns ``(X, elapsed)`` or ``X`` as
        ``solve_dga_batch_until``; ``tol``, ``targets`` and ``check_every`` are its stopping arguments, optional here: with ``tol``
        and ``targets`` both None the batch runs ``nb_iter`` iterations.

        ``X[k]`` and the k-th component of every curve are what ``solve(method="dual_gradient_ascent")`` gives on a copy of the LP
        whose ``costsvector`` is ``costs[k]`` and whose right-hand sides are row k (bit for bit); ``max_violated_constraint`` of
        instance k is taken against instance k's right-hand sides.  Sets ``self.dual_multipliers``, ``self.dual_lower_bounds``
        (each a certified lower bound on its instance's LP value) and ``self.stop_info``, the ``info`` of
        ``dual_gradient_ascent_batch_rhs``."""
        from .DualGradientAscent import _check_dga_batch_rhs_call, _dga_batch_rhs_run

        costs, batch = check_costs(costs, self.nb_variables)
        # the checks of dual_gradient_ascent_batch_rhs, made once and before the curves are touched
        stop, rhs = _check_dga_batch_rhs_call(self, costs, b_equalities, b_upper, tol, targets, check_every)
        start = time.perf_counter()
        _reset_curves(self)
        views = _rhs_views(self, batch, b_equalities=b_equalities, b_upper=b_upper)
        record = _batch_recorder(self, batch, ground_truth, ground_truth_indices, mean=_mean_each, views=views)
        x, y_eq, y_ineq, info = _dga_batch_rhs_run(self, costs, rhs, stop, nb_iter, record, None, None, max_time, lower_bounds, upper_bounds,
                                                   None)
        self.dual_multipliers = (y_eq, y_ineq)
        self.dual_lower_bounds = info["lower_bound"].copy()
        self.stop_info = info
        elapsed = time.perf_counter() - start
        return (x, elapsed) if get_timing else x

    def solve_dga_batch(
        self,
        costs,
        get_timing=True,
        nb_iter=10000,
        max_time=None,
        nb_iter_plot=10,
        ground_truth=None,
        ground_truth_indices=None,
        lower_bounds=None,
        upper_bounds=None,
    ):
        """Run ``method="dual_gradient_ascent"`` once for every row of ``costs`` (shape ``(B, nb_variables)``) in place of
        ``costsvector``, all B solves advancing together on the GPU (``DualGradientAscent.dual_gradient_ascent_batch``; extension:
        the reference solves one LP per call); returns ``(X, elapsed)`` or ``X``, ``X`` of shape ``(B, nb_variables)``.

        Constraints and right-hand sides are the LP's own; ``lower_bounds`` / ``upper_bounds`` (shape ``(nb_variables,)`` or
        ``(B, nb_variables)``) default to the LP's.  ``X[k]`` and the k-th component of every curve are what
        ``solve(method="dual_gradient_ascent")`` gives on a copy of the LP whose ``costsvector`` is ``costs[k]`` (bit for bit).
        Also sets ``self.dual_multipliers = (Y_eq, Y_ineq)`` and ``self.dual_lower_bounds`` of shape ``(B,)``: the dual energies of
        the returned multipliers, each a certified lower bound on its instance's LP value.  ``solve_batch(method=
        "dual_gradient_ascent")`` keeps refusing: it is the batched Chambolle-Pock only.

        Reports every 100 iterations whatever ``nb_iter_plot``, as the single method does.  ``itrn_curve``, ``opttime_curve``,
        ``dopttime_curve`` are lists of scalars; ``pobj_curve``, ``dobj_curve``, ``max_violated_equality``,
        ``max_violated_inequality``, ``max_violated_constraint`` (and, with ``ground_truth``, the two distance curves) are lists of
        arrays of length B (``max_violated_constraint`` is taken against the LP's own bounds).  ``max_time`` stops the whole batch.  Under a communicator every rank solves the whole batch (a replica).
        """
        from .DualGradientAscent import _dga_batch_run

        costs, batch = check_costs(costs, self.nb_variables)
        require_one_sided(self.b_lower)
        start = time.perf_counter()
        _reset_curves(self)

        record = _batch_recorder(self, batch, ground_truth, ground_truth_indices, mean=_mean_each)
        x, y_eq, y_ineq, report = _dga_batch_run(self, costs, nb_iter, record, None, None, max_time, lower_bounds, upper_bounds, None)
        self.dual_multipliers = (y_eq, y_ineq)
        self.dual_lower_bounds = report[:, 0].copy()
        elapsed = time.perf_counter() - start
        return (x, elapsed) if get_timing else x

    def solve_dga_batch_until(
        self,
        costs,
        tol=None,
        targets=None,
        check_every=10,
        get_timing=True,
        nb_iter=10000,
        max_time=None,
        nb_iter_plot=10,
        ground_truth=None,
        ground_truth_indices=None,
        lower_bounds=None,
        upper_bounds=None,
    ):
        """``solve_dga_batch`` with a stopping test per instance (``DualGradientAscent.dual_gradient_ascent_batch_until``): every
        instance stops on its own at the first iteration ``t`` with ``t % check_every == 0`` at which the step
        ``max|y_t - y_{t-1}|`` over its multipliers is at most ``tol`` or its certified lower bound, the dual energy of ``y_t``, has
        reached its cut-off ``targets[k]``; the others go on, at most ``nb_iter`` iterations.  Returns ``(X, elapsed)`` or ``X``.
        At least one of ``tol`` (a finite float ``>= 0``) and ``targets`` (a scalar or shape ``(B,)``, ``+inf`` for an instance
        without a cut-off) is required and ``check_every`` is an int ``>= 1``: a ``ValueError`` otherwise.

        Sets ``self.dual_multipliers`` and ``self.dual_lower_bounds`` as ``solve_dga_batch`` does, and ``self.stop_info``, the
        ``info`` of ``dual_gradient_ascent_batch_until``: a dict of arrays of length B, ``iterations``, ``stopped``, ``reason``,
        ``step`` and ``lower_bound``.  The curves are filled as by ``solve_dga_batch``, arrays of length B per report; the loop ends
        behind the first call after which no instance moves, and a stopped instance's entries are those of its final iterate.
        """
        from .DualGradientAscent import _check_batch_stop, _dga_batch_run

        costs, batch = check_costs(costs, self.nb_variables)
        stop = _check_batch_stop(tol, targets, check_every, batch)
        require_one_sided(self.b_lower)
        start = time.perf_counter()
        _reset_curves(self)

        record = _batch_recorder(self, batch, ground_truth, ground_truth_indices, mean=_mean_each)
        x, y_eq, y_ineq, info = _dga_batch_run(self, costs, nb_iter, record, None, None, max_time, lower_bounds, upper_bounds, None, stop=stop)
        self.dual_multipliers = (y_eq, y_ineq)
        self.dual_lower_bounds = info["lower_bound"].copy()
        self.stop_info = info
        elapsed = time.perf_counter() - start
        return (x, elapsed) if get_timing else x


def solve_many(lps, method="chambolle_pock_ppd", get_timing=True, nb_iter=10000, max_time=None, nb_iter_plot=10):
    """Solve a list of ``SparseLP`` objects whose matrices differ in ONE call, every LP one workgroup on the GPU (extension: the
    reference solves one LP per call); returns the list of ``x``, or ``(xs, elapsed)`` with ``get_timing``.

    Only ``method="chambolle_pock_ppd"`` exists in this form (``many_methods``; ``ChambollePockPPD.chambolle_pock_ppd_many``); any
    other raises ``ValueError`` -- for ``method="admm"`` on a list see ``solve_admm_many``, for dual gradient ascent
    ``solve_dga_many``.  Per LP the preparation is that of ``solve(setup="host")``: ``copy.deepcopy`` and
    ``remove_fixed_variables`` on the host (reference :1244-1248), ``x = m_change * sol - shift`` afterwards (:1259,:1288).
    ``xs[k]`` is bit for bit what ``lps[k].solve(method="chambolle_pock_ppd", order=ORDER_SEQUENTIAL, setup="host")`` returns.

    Fills every LP's curve attributes as ``solve`` does, at every report: ``itrn_curve``, ``opttime_curve``, ``dopttime_curve``,
    ``pobj_curve``, ``dobj_curve``, ``max_violated_constraint``, ``max_violated_equality``, ``max_violated_inequality``.
    ``max_time`` stops all LPs at a report.  Under a communicator every rank solves the whole list (a replica).
    """
    if method not in many_methods:
        raise ValueError(f"method {method!r} has no one-workgroup-per-LP form; solve_many supports: {many_methods}")
    lps = list(lps)
    if len(lps) < 1:
        raise ValueError("an empty list of LPs")
    start = time.perf_counter()
    problems, expand = _many_reduced(lps)
    sols, _ = chambolle_pock_ppd_many(problems, x0=None, alpha=1, theta=1, nb_max_iter=nb_iter, callback_func=_list_recorder(lps, expand),
                                      max_time=max_time, nb_iter_plot=nb_iter_plot)
    xs = [expand(k, sol) for k, sol in enumerate(sols)]
    elapsed = time.perf_counter() - start
    return (xs, elapsed) if get_timing else xs


def _many_reduced(lps):
    """The preparation of ``solve_many``: every LP's curves reset and its fixed variables removed on a copy.  Returns the
    solver's 8-tuples and ``expand(k, sol)``, the solver's iterate of LP ``k`` over the LP's own variables."""
    problems, maps = [], []
    for lp in lps:
        _reset_curves(lp)
        reduced = copy.deepcopy(lp)
        free, shift = reduced.remove_fixed_variables()
        if reduced.nb_variables < 1:
            raise ValueError("an LP of the list has no free variable (lower_bounds == upper_bounds everywhere)")
        maps.append((np.nonzero(free)[0], free.size, shift))
        problems.append((reduced.costsvector, reduced.a_equalities, reduced.b_equalities, reduced.a_inequalities, reduced.b_lower,
                         reduced.b_upper, reduced.lower_bounds, reduced.upper_bounds))

    def expand(k, sol):
        # reference :1259,:1288: x = m_change * sol - shift (note the sign it applies to the fixed values)
        free_ids, size, shift = maps[k]
        full = np.zeros(size)
        full[free_ids] = sol
        return full - shift

    return problems, expand


def solve_many_until(lps, tol, check_every=10, get_timing=True, nb_iter=10000, max_time=None, nb_iter_plot=10):
    """``solve_many`` with a stopping test per LP (``ChambollePockPPD.chambolle_pock_ppd_many_until``): every LP of the list stops
    on its own at the first iteration ``t`` with ``t % check_every == 0`` whose step ``max(max|x_t - x_{t-1}|, max|y_t -
    y_{t-1}|)`` is at most ``tol``, the others go on, at most ``nb_iter`` iterations.  Returns the list of ``x``, or ``(xs,
    elapsed)`` with ``get_timing``; ``tol`` a finite float ``>= 0`` and ``check_every`` an int ``>= 1``, a ``ValueError`` otherwise.

    The LPs are prepared as ``solve_many`` prepares them.  Sets ``lp.nb_iterations`` (iterations completed; for a stopped LP its
    stopping iteration) and ``lp.stopped`` on every LP.  A stopped LP records nothing after it has stopped, so for every LP,
    stopped or not, ``xs[k]`` and every curve apart from the times are bit for bit those of ``lps[k].solve(method=
    "chambolle_pock_ppd", nb_iter=lp.nb_iterations, order=ORDER_SEQUENTIAL, setup="host")`` (the energies to the rounding of
    another fixed summation order, as for ``solve_many``).  ``max_time`` stops all LPs at a report.
    """
    check_stop(tol, check_every)
    lps = list(lps)
    if len(lps) < 1:
        raise ValueError("an empty list of LPs")
    start = time.perf_counter()
    problems, expand = _many_reduced(lps)
    skip = np.zeros(len(lps), dtype=bool)
    fill = _list_recorder(lps, expand, skip=skip)

    def record(*report):
        skip[:] = record.info["stopped"]   # current at every callback: chambolle_pock_ppd_many_until sets the attribute
        fill(*report)

    sols, _, info = chambolle_pock_ppd_many_until(problems, tol, check_every, x0=None, alpha=1, theta=1, nb_max_iter=nb_iter,
                                                  callback_func=record, max_time=max_time, nb_iter_plot=nb_iter_plot)
    xs = [expand(k, sol) for k, sol in enumerate(sols)]
    for k, lp in enumerate(lps):
        lp.nb_iterations = int(info["iterations"][k])
        lp.stopped = bool(info["stopped"][k])
    elapsed = time.perf_counter() - start
    return (xs, elapsed) if get_timing else xs


def solve_many_certified(lps, tol_gap, tol_feas, check_every=10, get_timing=True, nb_iter=10000, max_time=None, nb_iter_plot=10):
    """``solve_many`` with a certificate as the stopping test per LP (``ChambollePockPPD.chambolle_pock_ppd_many_certified``): every
    LP of the list stops on its own at the first iteration ``t`` with ``t % check_every == 0`` at which its violation is at most
    ``tol_feas`` and the gap between its primal value and a valid lower bound is at most ``tol_gap * (1 + |primal| + |bound|)``;
    the others go on, at most ``nb_iter`` iterations.  Returns the list of ``x``, or ``(xs, elapsed)`` with ``get_timing``;
    ``tol_gap`` and ``tol_feas`` finite floats ``>= 0`` and ``check_every`` an int ``>= 1``, a ``ValueError`` otherwise.

    The LPs are prepared as ``solve_many`` prepares them.  Sets on every LP ``lp.nb_iterations`` (iterations completed; for a
    stopped LP its stopping iteration), ``lp.stopped``, and the last evaluated certificate: ``lp.primal_objective``,
    ``lp.lower_bound`` and ``lp.max_violation``.  These three are the numbers of the LP the solver holds, AFTER
    ``remove_fixed_variables``: the cost of the removed variables at their fixed values is not in them.  It is given separately
    as ``lp.fixed_cost``; add it to ``lp.primal_objective`` and to ``lp.lower_bound`` for the value and the bound of the LP as it
    was handed in.  As for ``solve_many_until`` a stopped LP records nothing after it has stopped, and ``xs[k]`` is bit for bit
    ``lps[k].solve(method="chambolle_pock_ppd", nb_iter=lp.nb_iterations, order=ORDER_SEQUENTIAL, setup="host")``.  ``max_time``
    stops all LPs at a report.
    """
    check_stop(tol_gap, check_every, "tol_gap")
    check_stop(tol_feas, check_every, "tol_feas")
    lps = list(lps)
    if len(lps) < 1:
        raise ValueError("an empty list of LPs")
    start = time.perf_counter()
    problems, expand = _many_reduced(lps)
    skip = np.zeros(len(lps), dtype=bool)
    fill = _list_recorder(lps, expand, skip=skip)

    def record(*report):
        skip[:] = record.info["stopped"]   # current at every callback: chambolle_pock_ppd_many_certified sets the attribute
        fill(*report)

    sols, _, info = chambolle_pock_ppd_many_certified(problems, tol_gap, tol_feas, check_every, x0=None, alpha=1, theta=1,
                                                      nb_max_iter=nb_iter, callback_func=record, max_time=max_time,
                                                      nb_iter_plot=nb_iter_plot)
    xs = [expand(k, sol) for k, sol in enumerate(sols)]
    for k, lp in enumerate(lps):
        lp.nb_iterations = int(info["iterations"][k])
        lp.stopped = bool(info["stopped"][k])
        lp.primal_objective = float(info["primal"][k])
        lp.lower_bound = float(info["lower_bound"][k])
        lp.max_violation = float(info["violation"][k])
        fixed = ~(lp.upper_bounds > lp.lower_bounds)
        lp.fixed_cost = float(np.dot(lp.costsvector[fixed], lp.lower_bounds[fixed]))
    elapsed = time.perf_counter() - start
    return (xs, elapsed) if get_timing else xs


def solve_dga_many(lps, get_timing=True, nb_iter=10000, max_time=None):
    """Run ``method="dual_gradient_ascent"`` on a list of ``SparseLP`` objects whose matrices differ in ONE call, every LP one
    workgroup on the GPU (``DualGradientAscent.dual_gradient_ascent_many``; extension: the reference solves one LP per call);
    returns the list of ``x``, or ``(xs, elapsed)`` with ``get_timing``.  Every LP has at most 8192 variables.

    ``xs[k]`` and every curve of ``lps[k]`` apart from the times are bit for bit what ``lps[k].solve(method=
    "dual_gradient_ascent")`` gives: a report every 100 iterations, none for an LP whose start is dual infeasible.  Also sets
    ``lp.dual_multipliers = (y_eq, y_ineq)`` and ``lp.dual_lower_bound`` on each LP: the dual energy of the returned multipliers,
    a certified lower bound on that LP's value.  ``solve_many(method="dual_gradient_ascent")`` keeps refusing: it is the
    Chambolle-Pock list form only.  ``max_time`` stops all LPs at a report.  Under a communicator every rank solves the whole
    list (a replica)."""
    from .DualGradientAscent import _dga_many_run

    lps = list(lps)
    if len(lps) < 1:
        raise ValueError("an empty list of LPs")
    start = time.perf_counter()
    for lp in lps:
        _reset_curves(lp)
    frozen = []   # a frozen LP records nothing: its single solve returns before the first report
    xs, y_eqs, y_ineqs, report, _ = _dga_many_run(lps, nb_iter, _list_recorder(lps, skip=frozen), None, None, max_time, frozen_out=frozen)
    for k, lp in enumerate(lps):
        lp.dual_multipliers = (y_eqs[k], y_ineqs[k])
        lp.dual_lower_bound = float(report[k, 0])
    elapsed = time.perf_counter() - start
    return (xs, elapsed) if get_timing else xs


def solve_dga_many_until(lps, tol, check_every=10, get_timing=True, nb_iter=10000, max_time=None):
    """``solve_dga_many`` with a stopping test per LP (``DualGradientAscent.dual_gradient_ascent_many_until``): every LP of the list
    stops on its own at the first iteration ``t`` with ``t % check_every == 0`` whose step ``max|y_t - y_{t-1}|`` over its
    multipliers is at most ``tol``, the others go on, at most ``nb_iter`` iterations.  Returns the list of ``x``, or ``(xs,
    elapsed)`` with ``get_timing``; ``tol`` a finite float ``>= 0`` and ``check_every`` an int ``>= 1``, a ``ValueError`` otherwise.

    Sets on every LP ``lp.nb_iterations`` (iterations completed; for a stopped LP its stopping iteration, 0 for an LP whose start
    is dual infeasible), ``lp.stopped``, ``lp.dual_multipliers = (y_eq, y_ineq)`` and ``lp.dual_lower_bound``, the dual energy of
    those multipliers: a certified lower bound on that LP's value.  A stopped LP records nothing after it has stopped, so for
    every LP ``xs[k]`` and every curve apart from the times are bit for bit those of ``lps[k].solve(method=
    "dual_gradient_ascent", nb_iter=lp.nb_iterations)``.  ``max_time`` stops all LPs at a report."""
    check_stop(tol, check_every)
    return _solve_dga_many_stopping(lps, tol, check_every, get_timing, nb_iter, max_time, None)


def solve_dga_many_cutoff(lps, tol, check_every=10, get_timing=True, nb_iter=10000, max_time=None, targets=None):
    """``solve_dga_many_until`` with a cut-off for each LP's certified lower bound as well
    (``DualGradientAscent.dual_gradient_ascent_many_cutoff``): an LP also stops at the first check at which the dual energy of its
    multipliers is ``>= targets[k]``.  ``tol`` may be None (no step test) when ``targets`` -- a scalar or one value per LP, ``+inf``
    for an LP without a cut-off -- is given; with ``targets`` None it is ``solve_dga_many_until``.  Bad arguments raise
    ``ValueError`` before the library is loaded.

    With ``targets`` it also sets ``lp.stop_reason`` (int bit mask: 0 not stopped, 1 step, 2 bound, 3 both at the same check).
    ``lp.dual_lower_bound`` stays the energy of the returned multipliers; for an LP stopped at a check with cut-offs it is, bit for
    bit, the bound that check evaluated."""
    return _solve_dga_many_stopping(lps, tol, check_every, get_timing, nb_iter, max_time, targets)


def solve_dga_many_compact(lps, tol, check_every=10, get_timing=True, nb_iter=10000, max_time=None, targets=None):
    """``solve_dga_many_cutoff`` with compaction on (``DualGradientAscent.dual_gradient_ascent_many_compact``): the LPs still
    moving are handed consecutive workgroups in every launch.  The same arguments, the same refusals before the library is loaded,
    the same ``xs`` and the same attributes on every LP, bit for bit; what changes is the time of a list in which LPs are retired
    here and there."""
    return _solve_dga_many_stopping(lps, tol, check_every, get_timing, nb_iter, max_time, targets, compact=True)


def _solve_dga_many_stopping(lps, tol, check_every, get_timing, nb_iter, max_time, targets, compact=False):
    """``solve_dga_many_until`` (``targets`` None), ``solve_dga_many_cutoff`` and, with ``compact``, ``solve_dga_many_compact``."""
    from .DualGradientAscent import _check_batch_stop, _dga_many_run

    lps = list(lps)
    if targets is None and tol is not None:
        stop, cutoff = check_stop(tol, check_every), None
    else:   # (both None: the refusal of _check_batch_stop)
        stop, cutoff = None, _check_batch_stop(tol, targets, check_every, len(lps))
    if len(lps) < 1:
        raise ValueError("an empty list of LPs")
    start = time.perf_counter()
    for lp in lps:
        _reset_curves(lp)
    frozen = []   # a frozen LP records nothing: its single solve returns before the first report
    skip = np.zeros(len(lps), dtype=bool)
    fill = _list_recorder(lps, skip=skip)

    def record(niter, *report):
        # the report of index niter belongs to iteration niter + 1: an LP that stopped before it has no such iteration
        info = record.info   # current at every callback: the driver sets the attribute
        skip[:] = np.asarray(frozen, dtype=bool) | (info["stopped"] & (info["iterations"] < niter + 1))
        fill(niter, *report)

    xs, y_eqs, y_ineqs, _, info = _dga_many_run(lps, nb_iter, record, None, None, max_time, frozen_out=frozen, stop=stop, cutoff=cutoff,
                                             compact=compact)
    for k, lp in enumerate(lps):
        lp.nb_iterations = int(info["iterations"][k])
        lp.stopped = bool(info["stopped"][k])
        if cutoff is not None:
            lp.stop_reason = int(info["reason"][k])
        lp.dual_multipliers = (y_eqs[k], y_ineqs[k])
        lp.dual_lower_bound = float(info["lower_bound"][k])
    elapsed = time.perf_counter() - start
    return (xs, elapsed) if get_timing else xs


def solve_admm_many(lps, get_timing=True, nb_iter=10000, max_time=None, nb_iter_plot=10):
    """Run ``method="admm"`` on a list of ``SparseLP`` objects whose matrices differ in ONE call, every LP one workgroup on the GPU
    (``ADMM.lp_admm_many``; extension: the reference solves one LP per call); returns the list of ``x``, or ``(xs, elapsed)`` with
    ``get_timing``.

    ``xs[k]`` and every curve of ``lps[k]`` apart from the times are what ``lps[k].solve(method="admm", order=ORDER_SEQUENTIAL,
    setup="host")`` gives: ``x`` and the violation curves bit for bit, the energies (``pobj_curve``, ``dobj_curve``) to the rounding
    of another fixed summation order.  No fixed variables are removed, as ``solve(method="admm")`` removes none.  An LP without
    inequality rows raises ``ValueError`` (the reference's standard form is undefined without them, tools.py:92).
    ``solve_many(method="admm")`` keeps refusing: it is the Chambolle-Pock list form only.  ``max_time`` stops all LPs at a
    report.  Under a communicator every rank solves the whole list (a replica)."""
    from .ADMM import lp_admm_many

    lps = list(lps)
    if len(lps) < 1:
        raise ValueError("an empty list of LPs")
    start = time.perf_counter()
    problems = _admm_many_prepared(lps)
    xs = lp_admm_many(problems, nb_iter=nb_iter, callback_func=_list_recorder(lps), max_time=max_time, nb_iter_plot=nb_iter_plot)
    elapsed = time.perf_counter() - start
    return (xs, elapsed) if get_timing else xs


def _admm_many_prepared(lps):
    """The preparation of ``solve_admm_many``: every LP's curves reset; returns the solver's 8-tuples."""
    problems = []
    for lp in lps:
        _reset_curves(lp)
        a_ineq = lp.a_inequalities if (lp.a_inequalities is not None and lp.a_inequalities.shape[0] > 0) else None
        a_eq, b_eq = (lp.a_equalities, lp.b_equalities) if lp.a_equalities.shape[0] > 0 else (None, None)
        problems.append((lp.costsvector, a_eq, b_eq, a_ineq, lp.b_lower, lp.b_upper, lp.lower_bounds, lp.upper_bounds))
    return problems


def solve_admm_many_until(lps, tol_residual, tol_step, check_every=10, get_timing=True, nb_iter=10000, max_time=None, nb_iter_plot=10):
    """``solve_admm_many`` with a stopping test per LP (``ADMM.lp_admm_many_until``): every LP of the list stops on its own at the
    first iteration ``t`` with ``t % check_every == 0`` at which ``max|A x_t - b| <= tol_residual`` (the rows of its standard form)
    and ``max|x_t - x_{t-1}| <= tol_step`` (all columns of it), the others go on, at most ``nb_iter + 1`` iterations.  Returns the
    list of ``x``, or ``(xs, elapsed)`` with ``get_timing``; both tolerances finite floats ``>= 0`` and ``check_every`` an int
    ``>= 1``, a ``ValueError`` otherwise.

    The LPs are prepared as ``solve_admm_many`` prepares them.  Sets ``lp.nb_iterations`` (iterations completed; for a stopped LP
    its stopping iteration) and ``lp.stopped`` on every LP.  A stopped LP records nothing after it has stopped, so ``xs[k]`` and
    every curve apart from the times are those of ``lps[k].solve(method="admm", nb_iter=lp.nb_iterations - 1,
    order=ORDER_SEQUENTIAL, setup="host")``: ``x`` and the violation curves bit for bit, the energies to the rounding of another
    fixed summation order, as for ``solve_admm_many``.  ``max_time`` stops all LPs at a report."""
    from .ADMM import lp_admm_many_until

    tol_residual, check_every = check_stop(tol_residual, check_every, "tol_residual")
    tol_step, _ = check_stop(tol_step, check_every, "tol_step")
    lps = list(lps)
    if len(lps) < 1:
        raise ValueError("an empty list of LPs")
    start = time.perf_counter()
    problems = _admm_many_prepared(lps)
    skip = np.zeros(len(lps), dtype=bool)
    fill = _list_recorder(lps, skip=skip)

    def record(*report):
        skip[:] = record.info["stopped"]   # current at every callback: lp_admm_many_until sets the attribute
        fill(*report)

    xs, info = lp_admm_many_until(problems, tol_residual, tol_step, check_every, nb_iter=nb_iter, callback_func=record, max_time=max_time,
                                  nb_iter_plot=nb_iter_plot)
    for k, lp in enumerate(lps):
        lp.nb_iterations = int(info["iterations"][k])
        lp.stopped = bool(info["stopped"][k])
    elapsed = time.perf_counter() - start
    return (xs, elapsed) if get_timing else xs
