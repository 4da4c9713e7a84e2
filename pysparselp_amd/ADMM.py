"""ADMM LP solver: host driver over the HIP kernels.

Drop-in for ``pysparselp.ADMM.lp_admm`` (reference ADMM.py:47-269) as shipped,
i.e. with the x-step solved by ONE sweep of box-projected Gauss-Seidel on the
explicit ``M = gamma_eq A^T A + gamma_ineq I`` (flags at ADMM.py:66-71).  Same
signature, callback contract and return value (the first ``n`` entries of the
standard-form iterate).

The two constraint blocks are uploaded once, as the caller holds them; the whole
setup chain of ADMM.py:73-101 -- row normalisation of each block, slack standard
form, row normalisation of the stacked system, ``M = gamma_eq A^T A + gamma_ineq I``
and ``A^T b`` -- runs on the device (``slp_admm_create_lp``, csrc/slp_spgemm.hip)
with scipy's entry orders and accumulation orders, so the state is bit-identical
to the reference's.  (``SLP_HOST_SETUP=1`` prepares the same arrays with the numpy
restatement in tools.py instead and uploads them; the tests compare the two.)
Only the level schedule of the Gauss-Seidel sweep is planned on the host, from
one download of ``M``.  The loop -- right-hand side with ``A^T lambda``, the
level-scheduled Gauss-Seidel sweep, the multiplier update with ``A x`` and the
report reductions -- runs on the GPU (csrc/slp_admm.hip).
"""
import os
import time

import numpy as np

from . import _lib
from . import _many
from ._admm_gap import ADMMGapMethods, gap_info
from ._batch import check_rhs, check_rhs_order, concat, first_offsets, shared_or_batched
from ._lib import ORDER_AUTO
from .tools import convert_to_standard_form_with_bounds, normal_matrix, precondition_constraints


class ADMMState(ADMMGapMethods):
    """Device-resident ADMM state (thin RAII wrapper of ``slp_admm``).  ``certificate``, ``set_stop_gap`` and ``gap_state`` are
    ``_admm_gap.ADMMGapMethods``'."""

    def __init__(self, a, b, c, lb, ub, x0, m, gamma_eq, gamma_ineq, order=ORDER_AUTO):
        """``m``: the explicit ``M`` (CSR arrays) or ``None`` to have it formed on the device from ``a``."""
        self._l = _lib.lib()
        self.N = a.shape[1]
        self.m = a.shape[0]
        b, c, lb, ub, x0 = (_lib.f64(v) for v in (b, c, lb, ub, x0))
        assert b.size == self.m and c.size == self.N and lb.size == self.N and ub.size == self.N and x0.size == self.N
        self._h = _lib.check_handle(self._l.slp_admm_create(
            self.N, self.m, _lib.ptr(a.indptr), _lib.ptr(a.indices), _lib.ptr(a.data), _lib.ptr(b), _lib.ptr(c),
            _lib.ptr(lb), _lib.ptr(ub), _lib.ptr(x0), *((None, None, None) if m is None else (_lib.ptr(m.indptr), _lib.ptr(m.indices), _lib.ptr(m.data))),
            float(gamma_eq), float(gamma_ineq), int(order)))

    @classmethod
    def from_lp(cls, c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0, gamma_eq, gamma_ineq, use_preconditioning=True,
                order=ORDER_AUTO):
        """The solver state from the LP as ``lp_admm`` receives it; all setup transforms run on the device."""
        from .tools import CsrArrays

        self = cls.__new__(cls)
        self._l = _lib.lib()
        a_eq, a_ineq = CsrArrays.from_any(a_eq), CsrArrays.from_any(a_ineq)
        if a_ineq is None:  # what the reference does on this input (tools.py:92-127)
            raise UnboundLocalError("local variable 'a_eq2' referenced before assignment (no inequality constraints)")
        n = a_ineq.shape[1]
        c, lb, ub = _lib.f64(c), _lib.f64(lb), _lib.f64(ub)
        m_eq = a_eq.shape[0] if a_eq is not None else 0
        m_ineq = a_ineq.shape[0]
        self.N, self.m = n + m_ineq, m_eq + m_ineq
        opt = lambda v: None if v is None else _lib.f64(v)  # noqa: E731
        beq, b_lower, b_upper, x0 = opt(beq), opt(b_lower), opt(b_upper), opt(x0)
        eq = (None, None, None) if a_eq is None else (_lib.ptr(a_eq.indptr), _lib.ptr(a_eq.indices), _lib.ptr(a_eq.data))
        self._h = _lib.check_handle(self._l.slp_admm_create_lp(
            n, m_eq, *eq, _lib.ptr(beq), m_ineq, _lib.ptr(a_ineq.indptr), _lib.ptr(a_ineq.indices), _lib.ptr(a_ineq.data),
            _lib.ptr(b_lower), _lib.ptr(b_upper), _lib.ptr(c), _lib.ptr(lb), _lib.ptr(ub), _lib.ptr(x0), float(gamma_eq),
            float(gamma_ineq), int(bool(use_preconditioning)), int(order)))
        return self

    def close(self):
        if getattr(self, "_h", None):
            self._l.slp_admm_destroy(self._h)
            self._h = None

    __del__ = close

    def set_xstep(self, mode):
        _lib.check(self._l.slp_admm_set_xstep(self._h, int(mode)))

    def iterate(self, k):
        _lib.check(self._l.slp_admm_iterate(self._h, int(k)))

    def sweep_step(self):
        _lib.check(self._l.slp_admm_sweep_step(self._h))

    def multiplier_step(self):
        _lib.check(self._l.slp_admm_multiplier_step(self._h))

    def report(self):
        out = np.zeros(4)
        _lib.check(self._l.slp_admm_report(self._h, _lib.ptr(out)))
        return out

    def x(self, count=None):
        count = self.N if count is None else int(count)
        out = np.empty(count)
        _lib.check(self._l.slp_admm_get_x(self._h, _lib.ptr(out), count))
        return out

    def lam(self):
        out = np.empty(self.m)
        _lib.check(self._l.slp_admm_get_lambda(self._h, _lib.ptr(out)))
        return out

    def num_levels(self):
        return int(self._l.slp_admm_num_levels(self._h))

    def num_bands(self):
        """Workgroups sharing the runs of narrow levels of M's Gauss-Seidel plan (0: one workgroup per run)."""
        return int(self._l.slp_admm_num_bands(self._h))

    def bench(self, k):
        ms = np.zeros(1)
        _lib.check(self._l.slp_admm_bench(self._h, int(k), _lib.ptr(ms)))
        return float(ms[0])


def lp_admm(
    c,
    a_eq,
    beq,
    a_ineq,
    b_lower,
    b_upper,
    lb,
    ub,
    x0=None,
    gamma_eq=2,
    gamma_ineq=3,
    nb_iter=100,
    callback_func=None,
    max_time=None,
    use_preconditioning=True,
    nb_iter_plot=10,
    order=ORDER_AUTO,
    xstep="gauss_seidel",
    setup="auto",
):
    """minimise c.x  s.t.  a_eq x = beq,  b_lower <= a_ineq x <= b_upper,  lb <= x <= ub.

    ``xstep`` (extension): ``"gauss_seidel"`` is the reference as shipped;
    ``"cg"`` is the reference's conjugate-gradient branch (flags at
    ADMM.py:66-71), run matrix-free -- see ``admm_cg.py``;
    ``"gauss_seidel_unbounded"`` is its plain Gauss-Seidel + over-relaxation
    branch (ADMM.py:164-181).
    ``setup`` (extension, ``xstep="cg"`` only): where its set-up chain runs,
    ``"auto"`` / ``"host"`` / ``"device"`` -- see ``admm_cg.lp_admm_cg``.
    """
    return _admm_run(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0, gamma_eq, gamma_ineq, nb_iter, callback_func, max_time,
                     use_preconditioning, nb_iter_plot, order, xstep, setup)[0]


def _admm_run(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0, gamma_eq, gamma_ineq, nb_iter, callback_func, max_time,
              use_preconditioning, nb_iter_plot, order, xstep, setup, gap=None):
    """``lp_admm`` (``gap`` None) and ``lp_admm_certified`` (``gap`` the checked ``(tol_gap, tol_feas, check_every)``): ``(x, info)``,
    ``info`` None without a test."""
    if xstep == "cg":
        from .admm_cg import _admm_cg_run

        return _admm_cg_run(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0, gamma_eq, gamma_ineq, nb_iter, callback_func, max_time,
                            use_preconditioning, nb_iter_plot, order, False, setup, gap)
    if xstep not in ("gauss_seidel", "gauss_seidel_unbounded"):
        raise ValueError(f"unknown xstep {xstep!r}")
    c = _lib.f64(c)
    n = c.size
    if os.environ.get("SLP_HOST_SETUP") == "1":
        # the numpy restatement of the setup chain (tools.py), then one upload of the finished arrays
        if x0 is None:
            x0 = np.zeros(n)
        if a_eq is not None:
            a_eq, beq = precondition_constraints(a_eq, beq, alpha=2)
        if a_ineq is not None:
            a_ineq, b_lower, b_upper = precondition_constraints(a_ineq, b_lower, b_upper, alpha=2)
        c2, a, b, lb2, ub2, x_init = convert_to_standard_form_with_bounds(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0)
        if use_preconditioning:
            a, b = precondition_constraints(a, b, alpha=2)
        m_mat = normal_matrix(a, gamma_eq, gamma_ineq) if os.environ.get("SLP_HOST_SPGEMM") == "1" else None
        state = ADMMState(a, b, c2, lb2, ub2, x_init, m_mat, gamma_eq, gamma_ineq, order)
    else:
        # ADMM.py:76-101 on the device: blocks uploaded once, nothing else crosses PCIe but M's download for the level plan
        state = ADMMState.from_lp(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0, gamma_eq, gamma_ineq, use_preconditioning, order)
    if xstep == "gauss_seidel_unbounded":  # the reference's use_unbounded_gauss_siedel flags (ADMM.py:164-181)
        state.set_xstep(1)
    try:
        if gap is not None:
            state.set_stop_gap(*gap)
        start = time.perf_counter()
        i = 0
        while i <= nb_iter:  # ADMM.py:143: nb_iter + 1 sweeps
            if i % nb_iter_plot == 0:
                # a stopped state ignores iterate, so i may run ahead of the state's own count until this report finds it stopped
                if gap is not None and state.gap_state()[1]:
                    break
                state.sweep_step()
                elapsed = time.perf_counter() - start
                if max_time is not None and elapsed > max_time:
                    break
                energy1, max_violated_equality, max_violated_inequality = state.report()[:3]
                if callback_func is not None:
                    callback_func(i, state.x(n), energy1, energy1, elapsed, max_violated_equality, max_violated_inequality)
                state.multiplier_step()
                i += 1
            else:
                k = min(nb_iter_plot - i % nb_iter_plot, nb_iter + 1 - i)
                state.iterate(k)
                i += k
        return state.x(n), None if gap is None else gap_info(state)
    finally:
        state.close()


def lp_admm_certified(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, tol_gap, tol_feas, check_every=10, x0=None, gamma_eq=2,
                      gamma_ineq=3, nb_iter=100, callback_func=None, max_time=None, use_preconditioning=True, nb_iter_plot=10,
                      order=ORDER_AUTO, xstep="gauss_seidel", setup="auto"):
    """``lp_admm`` that stops on a certificate (extension; the reference stops on nothing): at the first iteration ``t`` with
    ``t % check_every == 0`` at which the violation of ``x_t`` is at most ``tol_feas`` and the gap between ``c.x_t`` and a valid
    lower bound is at most ``tol_gap * (1 + |primal| + |bound|)`` (``ADMMState.set_stop_gap``), or after the ``nb_iter + 1``
    iterations of ``lp_admm``.  Every ``xstep`` and ``setup`` of ``lp_admm``, and the row partition of ``xstep="cg"`` under a
    communicator.

    Returns ``(x, info)``; ``info`` is a dict of ``iterations`` (whole iterations completed), ``stopped``, and the last evaluated
    certificate ``primal``, ``lower_bound``, ``violation`` (``+inf``, ``-inf``, ``+inf`` before the first check).  The three numbers
    belong to the standard form the solver holds: ``violation`` is in its row-normalised units, those of the callback's
    ``max_violated_equality``, not in the caller's.  ``x`` is bit for bit ``lp_admm(..., nb_iter=info["iterations"] - 1)``.  The
    callback cadence is that of ``lp_admm``; the loop ends, without a report, at the first report that finds the state stopped.
    ``tol_gap`` and ``tol_feas`` finite floats ``>= 0`` and ``check_every`` an int ``>= 1``: a ``ValueError`` otherwise, before
    anything is uploaded."""
    from ._cp_gap import check_gap

    gap = check_gap(tol_gap, tol_feas, check_every)
    return _admm_run(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0, gamma_eq, gamma_ineq, nb_iter, callback_func, max_time,
                     use_preconditioning, nb_iter_plot, order, xstep, setup, gap)


# ---------------------------------------------------------------------------------------------------------------------
# batched form: B LPs over one constraint structure
def _validate_batch(cs, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0):
    """Everything ``lp_admm_batch`` can refuse without a GPU; returns the arguments as contiguous float64 arrays / CSR triples."""
    from .tools import CsrArrays

    cs = np.asarray(cs, dtype=np.float64)
    if cs.ndim != 2:
        raise ValueError(f"cs has shape {cs.shape}: expected (B, n), one row of costs per instance")
    batch, n = cs.shape
    if batch < 1:
        raise ValueError("an empty batch: cs needs at least one row (B >= 1)")
    if n < 1:
        raise ValueError(f"cs has shape {cs.shape}: the LP needs at least one variable")
    if not np.all(np.isfinite(cs)):
        k = int(np.nonzero(~np.all(np.isfinite(cs), axis=1))[0][0])
        raise ValueError(f"instance {k} has a cost that is not finite")
    for name, v in (("beq", beq), ("b_lower", b_lower), ("b_upper", b_upper)):
        if v is not None and np.ndim(v) != 1:
            raise ValueError(f"{name} has shape {np.shape(v)}: the right-hand sides are shared by the instances of a batch "
                             "(per-instance right-hand sides are not built)")
    a_eq, a_ineq = CsrArrays.from_any(a_eq), CsrArrays.from_any(a_ineq)
    if a_ineq is None:
        raise ValueError("no inequality block: the reference cannot form the standard form without one (tools.py:92)")
    for name, a in (("a_eq", a_eq), ("a_ineq", a_ineq)):
        if a is not None:
            if a.shape[1] != n:
                raise ValueError(f"{name} has {a.shape[1]} columns, cs has {n}")
            if a.indices.size and (a.indices.min() < 0 or a.indices.max() >= n):
                raise ValueError(f"{name} has a column index outside [0, {n})")
    m_eq, m_ineq = (0 if a_eq is None else a_eq.shape[0]), a_ineq.shape[0]

    def rhs(name, v, rows):
        if v is None:
            return None
        v = _lib.f64(v)
        if v.shape != (rows,):
            raise ValueError(f"{name} has shape {v.shape}: expected ({rows},)")
        if np.any(np.isnan(v)):
            raise ValueError(f"{name} has a NaN")
        return v

    beq = rhs("beq", beq, m_eq) if a_eq is not None else None
    if a_eq is not None and beq is None:
        raise ValueError("a_eq without beq")
    b_lower, b_upper = rhs("b_lower", b_lower, m_ineq), rhs("b_upper", b_upper, m_ineq)
    lb, lb_b = shared_or_batched("lb", lb, batch, n)
    ub, ub_b = shared_or_batched("ub", ub, batch, n)
    if np.any(np.isnan(lb)) or np.any(np.isnan(ub)):
        raise ValueError("lb / ub has a NaN")
    x0_b = False
    if x0 is not None:
        x0, x0_b = shared_or_batched("x0", x0, batch, n)
        if not np.all(np.isfinite(x0)):
            raise ValueError("x0 has an entry that is not finite")
    return np.ascontiguousarray(cs), a_eq, beq, a_ineq, b_lower, b_upper, lb, lb_b, ub, ub_b, x0, x0_b


def _check_batch_rhs(batch, m_eq, m_ineq, beq, b_lower, b_upper, kept_lower=None, kept_upper=None):
    """The sides of ``ADMMBatchState.set_rhs`` checked without the library: each None or a contiguous float64 array of shape
    ``(rows,)`` or ``(batch, rows)``; a side of a block without rows becomes None.  ``kept_lower`` / ``kept_upper``: what the other
    side of the inequality block is compared against when only one is given."""
    beq = None if beq is None or m_eq == 0 else check_rhs("beq", beq, batch, m_eq, finite=True)[0]
    if beq is not None and beq.ndim == 1 and not np.all(np.isfinite(beq)):
        raise ValueError("beq has an entry that is not finite")
    b_lower = None if b_lower is None or m_ineq == 0 else check_rhs("b_lower", b_lower, batch, m_ineq)[0]
    b_upper = None if b_upper is None or m_ineq == 0 else check_rhs("b_upper", b_upper, batch, m_ineq)[0]
    if b_lower is not None or b_upper is not None:
        check_rhs_order(kept_lower if b_lower is None else b_lower, kept_upper if b_upper is None else b_upper, batch)
    return beq, b_lower, b_upper


class ADMMBatchState:
    """Device-resident batched ADMM state (thin RAII wrapper of ``slp_admm_batch``): ``cs`` is ``(B, n)``; ``lb``, ``ub``, ``x0``
    are shared vectors or carry a leading axis ``B``; the constraint blocks are shared, and so are their right-hand sides until
    ``set_rhs`` gives every instance its own."""

    def __init__(self, cs, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0=None, gamma_eq=2, gamma_ineq=3, use_preconditioning=True):
        cs, a_eq, beq, a_ineq, b_lower, b_upper, lb, lb_b, ub, ub_b, x0, x0_b = _validate_batch(cs, a_eq, beq, a_ineq, b_lower, b_upper,
                                                                                                lb, ub, x0)
        self.batch, self.n = cs.shape
        m_eq = a_eq.shape[0] if a_eq is not None else 0
        m_ineq = a_ineq.shape[0]
        self.N, self.m = self.n + m_ineq, m_eq + m_ineq
        self.m_eq, self.m_ineq = m_eq, m_ineq
        self._b_lower, self._b_upper = b_lower, b_upper   # what set_rhs compares a new side against
        eq = (None, None, None) if a_eq is None else (_lib.ptr(a_eq.indptr), _lib.ptr(a_eq.indices), _lib.ptr(a_eq.data))
        # all of the above needs no GPU; the library is loaded (and bound to a device) only now
        self._l = _lib.lib()
        self._h = _lib.check_handle(self._l.slp_admm_batch_create_lp(
            self.n, m_eq, *eq, _lib.ptr(beq), m_ineq, _lib.ptr(a_ineq.indptr), _lib.ptr(a_ineq.indices), _lib.ptr(a_ineq.data),
            _lib.ptr(b_lower), _lib.ptr(b_upper), self.batch, _lib.ptr(cs), 1, _lib.ptr(lb), int(lb_b), _lib.ptr(ub), int(ub_b),
            _lib.ptr(x0), int(x0_b), float(gamma_eq), float(gamma_ineq), int(bool(use_preconditioning))))

    def close(self):
        if getattr(self, "_h", None):
            self._l.slp_admm_batch_destroy(self._h)
            self._h = None

    __del__ = close

    def iterate(self, k):
        _lib.check(self._l.slp_admm_batch_iterate(self._h, int(k)))

    def sweep_step(self):
        _lib.check(self._l.slp_admm_batch_sweep_step(self._h))

    def multiplier_step(self):
        _lib.check(self._l.slp_admm_batch_multiplier_step(self._h))

    def report(self):
        """``(B, 3)``: augmented-Lagrangian energy, max |A x - b|, max(0, -min x) per instance."""
        out = np.zeros((self.batch, 3))
        _lib.check(self._l.slp_admm_batch_report(self._h, _lib.ptr(out)))
        return out

    def set_rhs(self, beq=None, b_lower=None, b_upper=None):
        """Replaces right-hand sides (``slp_admm_batch_set_rhs``): ``beq`` of shape ``(m_eq,)`` or ``(B, m_eq)``, ``b_lower`` and
        ``b_upper`` of shape ``(m_ineq,)`` or ``(B, m_ineq)``, in the units of the constructor; None keeps what the state has.  The
        library scales them with the row scalings of the shared set-up chain and rebuilds, per instance, ``b``, ``q`` and the slack
        part of ``lb`` / ``ub``, so instance k is bit for bit ``lp_admm(..., order=ORDER_SEQUENTIAL)`` on row k.  Only before the
        first iteration or half iteration (``SlpError`` afterwards, the state keeps what it had); may be called more than once.  A
        wrong shape, a NaN, an infinite entry of a batched ``beq`` or ``b_lower[k] > b_upper[k]`` on a row (both name the instance)
        is a ``ValueError`` before the library is touched."""
        return self._set_rhs(*_check_batch_rhs(self.batch, self.m_eq, self.m_ineq, beq, b_lower, b_upper, self._b_lower, self._b_upper))

    def _set_rhs(self, beq, b_lower, b_upper):
        """``set_rhs`` with sides that ``_check_batch_rhs`` has checked."""
        args = []
        for v in (beq, b_lower, b_upper):
            args += [_lib.ptr(v), 0 if v is None else int(v.ndim == 2)]
        _lib.check(self._l.slp_admm_batch_set_rhs(self._h, *args))
        # only now: after a refusal the state, and what a later call is compared against, keep the sides they had
        if b_lower is not None:
            self._b_lower = b_lower
        if b_upper is not None:
            self._b_upper = b_upper

    def set_stop(self, tol_residual, tol_step, check_every=1):
        """Arms the per-instance stopping test of the iteration kernels (``slp_admm_batch_set_stop``): at the end of every
        iteration ``t`` of the state with ``t % check_every == 0`` -- counted from 1 over the state's life; an iteration is the
        right-hand side, the sweep and the multiplier update -- a running instance stops iff ``max|A x_t - b| <= tol_residual``
        (the rows of the standard form) and ``max|x_t - x_{t-1}| <= tol_step`` (all ``N`` columns, slacks included); it keeps its
        iterate while the others go on.  The batch has one iteration counter, so a stopped instance stays stopped for the life of
        the state: a further call changes tolerances and cadence for the running instances and keeps the flags, and
        ``tol_residual=None`` turns the test off for them.  Between whole iterations only (not between ``sweep_step`` and
        ``multiplier_step``)."""
        if tol_residual is None:
            tol_residual, tol_step, check_every = -1.0, 0.0, 1
        else:
            tol_residual, check_every = _many.check_stop(tol_residual, check_every, "tol_residual")
            tol_step, _ = _many.check_stop(tol_step, check_every, "tol_step")
        _lib.check(self._l.slp_admm_batch_set_stop(self._h, tol_residual, tol_step, check_every))

    def stop_state(self):
        """``(iterations, stopped, residual, step)`` per instance, int64, bool and two float64 arrays: the iterations completed
        (for a stopped instance its stopping iteration), whether it is stopped -- for the life of the state -- and the last
        evaluated residual and step (``+inf`` before the first test)."""
        iterations, stopped = np.zeros(self.batch, dtype=np.int64), np.zeros(self.batch, dtype=np.int32)
        residual, step = np.zeros(self.batch), np.zeros(self.batch)
        _lib.check(self._l.slp_admm_batch_stop_state(self._h, _lib.ptr(iterations), _lib.ptr(stopped), _lib.ptr(residual), _lib.ptr(step)))
        return iterations, stopped.astype(bool), residual, step

    def x(self, count=None):
        count = self.N if count is None else int(count)
        out = np.empty((self.batch, count))
        _lib.check(self._l.slp_admm_batch_get_x(self._h, _lib.ptr(out), count))
        return out

    def lam(self):
        out = np.empty((self.batch, self.m))
        _lib.check(self._l.slp_admm_batch_get_lambda(self._h, _lib.ptr(out)))
        return out

    def num_levels(self):
        return int(self._l.slp_admm_batch_num_levels(self._h))

    def form(self):
        """``"tile"`` (one workgroup per tile of instances runs whole iterations) or ``"levels"`` (one launch per level)."""
        return ("tile", "levels")[int(self._l.slp_admm_batch_form(self._h))]

    def bench(self, k):
        """GPU milliseconds per batched iteration over ``k`` iterations (HIP events)."""
        ms = np.zeros(1)
        _lib.check(self._l.slp_admm_batch_bench(self._h, int(k), _lib.ptr(ms)))
        return float(ms[0])


def lp_admm_batch(
    cs,
    a_eq,
    beq,
    a_ineq,
    b_lower,
    b_upper,
    lb,
    ub,
    x0=None,
    gamma_eq=2,
    gamma_ineq=3,
    nb_iter=100,
    callback_func=None,
    max_time=None,
    use_preconditioning=True,
    nb_iter_plot=10,
):
    """``lp_admm`` for B LPs at once (extension; the reference solves one LP per call): minimise ``cs[k].x``  s.t.
    ``a_eq x = beq``, ``b_lower <= a_ineq x <= b_upper``, ``lb[k] <= x <= ub[k]`` for every k.

    ``cs`` has shape ``(B, n)``; ``lb``, ``ub`` and ``x0`` each have shape ``(n,)`` (shared by all instances) or ``(B, n)``.
    The right-hand sides are shared: a 2-D ``beq``, ``b_lower`` or ``b_upper`` raises ``ValueError`` (right-hand sides per
    instance are what ``lp_admm_batch_rhs`` takes), like every shape, finiteness and column-index error, before anything is
    uploaded.  The instances
    share the whole set-up chain (ADMM.py:73-101), ``M`` and its Gauss-Seidel plan; every instance is bit for bit what
    ``lp_admm(..., order=ORDER_SEQUENTIAL)`` computes for it.

    The loop is that of ``lp_admm``: ``nb_iter + 1`` sweeps, a report after those with ``i % nb_iter_plot == 0`` --
    ``callback_func(i, X, energy, energy, elapsed, max_violated_equality, max_violated_inequality)`` with ``X`` of shape
    ``(B, n)`` and arrays of length B; ``max_time`` stops the whole batch at a report.  Returns ``X``.

    Under a communicator every rank solves the whole batch (a replica).
    """
    X, _ = _admm_batch_run(cs, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0, gamma_eq, gamma_ineq, nb_iter, callback_func, max_time,
                           use_preconditioning, nb_iter_plot, None)
    return X


def _admm_batch_run(cs, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0, gamma_eq, gamma_ineq, nb_iter, callback_func, max_time,
                    use_preconditioning, nb_iter_plot, stop, rhs=None):
    """``lp_admm_batch`` (``stop`` None) and ``lp_admm_batch_until`` (``stop`` the checked ``(tol_residual, tol_step,
    check_every)``): ``(X, info)``, ``info`` None without a stopping test.  ``rhs``: the checked ``(beq, b_lower, b_upper)`` of
    ``lp_admm_batch_rhs``, handed to ``set_rhs`` before the first iteration."""
    state = ADMMBatchState(cs, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0, gamma_eq, gamma_ineq, use_preconditioning)
    if rhs is not None:
        try:
            state._set_rhs(*rhs)
        except BaseException:
            state.close()
            raise
    n = state.n
    solved = np.arange(state.batch)  # every instance takes part
    info = None if stop is None else _many.new_stop_info(state.batch, solved, residual=True)

    def stopped_now():
        now = state.stop_state()
        _many.spread_stop_state(info, solved, now)
        return now[1]

    try:
        if stop is not None:
            state.set_stop(*stop)
            if callback_func is not None:
                try:
                    callback_func.info = info
                except AttributeError:   # a bound method takes no attribute: wrap it in a function to read ``info``
                    pass
        start = time.perf_counter()
        i = 0
        while i <= nb_iter:  # ADMM.py:143: nb_iter + 1 sweeps
            if i % nb_iter_plot == 0:
                if stop is not None and stopped_now().all():
                    break
                state.sweep_step()
                elapsed = time.perf_counter() - start
                if max_time is not None and elapsed > max_time:
                    break
                energy, max_violated_equality, max_violated_inequality = state.report().T.copy()
                if callback_func is not None:
                    callback_func(i, state.x(n), energy, energy.copy(), elapsed, max_violated_equality, max_violated_inequality)
                state.multiplier_step()
                i += 1
            else:
                k = min(nb_iter_plot - i % nb_iter_plot, nb_iter + 1 - i)
                state.iterate(k)
                i += k
        if stop is not None:
            stopped_now()
        return state.x(n), info
    finally:
        state.close()


def lp_admm_batch_until(
    cs,
    a_eq,
    beq,
    a_ineq,
    b_lower,
    b_upper,
    lb,
    ub,
    tol_residual,
    tol_step,
    check_every=10,
    x0=None,
    gamma_eq=2,
    gamma_ineq=3,
    nb_iter=10000,
    callback_func=None,
    max_time=None,
    use_preconditioning=True,
    nb_iter_plot=10,
):
    """``lp_admm_batch`` with a stopping test per instance (extension; the reference has no stopping test): the batch runs until
    every instance has stopped, at most ``nb_iter + 1`` sweeps.  Returns ``(X, info)``.

    The test is made inside the iteration kernels (``ADMMBatchState.set_stop``), at the end of every iteration ``t`` of the batch
    with ``t % check_every == 0``, iterations counted from 1: an instance stops iff ``max|A x_t - b| <= tol_residual``, over the
    rows of the standard form and with the very residual the multiplier update forms, and ``max|x_t - x_{t-1}| <= tol_step``,
    over all ``n + m_ineq`` columns of the standard form; a NaN in either never stops.  A stopped instance keeps ``x_t`` and
    ``lambda_t``, bit for bit those of ``lp_admm(..., nb_iter=t - 1, order=ORDER_SEQUENTIAL)``, while the others go on.
    ``tol_residual`` and ``tol_step`` are finite floats ``>= 0``, ``check_every`` an int ``>= 1``: a ``ValueError`` that names
    the argument, before the library is loaded, otherwise, like every shape error.

    ``info`` is the dict of ``lp_admm_many_until``, of arrays over the batch: ``iterations`` (int64: completed, for a stopped
    instance its stopping iteration), ``stopped`` (bool), ``residual`` and ``step`` (float64: the last evaluated ones, ``+inf``
    before the first test).

    The loop and the cadence of reports are those of ``lp_admm_batch``: a report at index ``i`` lies between sweep ``i + 1`` and
    its multiplier update.  The loop ends at the first report index at which every instance is stopped (no callback for that
    index), at ``nb_iter``, or at ``max_time``.  In a callback a stopped instance's row of ``X`` is its final iterate and its
    three numbers are the report on that frozen state, so its ``max_violated_equality`` equals ``info["residual"][k]`` exactly.
    ``info`` is current at every callback: the same dict, updated in place, is set as the ATTRIBUTE ``callback_func.info`` before
    the first call (a function or any object that takes attributes; a bound method takes none and has to be wrapped in a
    function to read it).
    """
    tol_residual, check_every = _many.check_stop(tol_residual, check_every, "tol_residual")
    tol_step, _ = _many.check_stop(tol_step, check_every, "tol_step")
    return _admm_batch_run(cs, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0, gamma_eq, gamma_ineq, nb_iter, callback_func, max_time,
                           use_preconditioning, nb_iter_plot, (tol_residual, tol_step, check_every))


def lp_admm_batch_rhs(
    cs,
    a_eq,
    beq,
    a_ineq,
    b_lower,
    b_upper,
    lb,
    ub,
    tol_residual=None,
    tol_step=None,
    check_every=10,
    x0=None,
    gamma_eq=2,
    gamma_ineq=3,
    nb_iter=100,
    callback_func=None,
    max_time=None,
    use_preconditioning=True,
    nb_iter_plot=10,
):
    """``lp_admm_batch`` / ``lp_admm_batch_until`` with right-hand sides per instance (extension): ``beq`` has shape ``(m_eq,)`` or
    ``(B, m_eq)``, ``b_lower`` and ``b_upper`` ``(m_ineq,)`` or ``(B, m_ineq)`` (or None: no such bound) -- a sweep over
    capacities, budgets or demands.  Returns ``(X, info)``; ``info`` is None without tolerances.

    The row scalings of the set-up chain depend on the matrices only, so the instances still share the chain, ``M`` and its
    Gauss-Seidel plan; ``ADMMBatchState.set_rhs`` builds every instance's ``b``, ``q`` and slack bounds on the device.  Instance k
    is bit for bit ``lp_admm(cs[k], a_eq, beq[k], a_ineq, b_lower[k], b_upper[k], ..., order=ORDER_SEQUENTIAL)``.  The loop, the
    reports and ``callback_func`` are those of ``lp_admm_batch``; the energies and violations handed to the callback are each
    instance's own, against its own right-hand sides.  With ``tol_residual`` and ``tol_step`` (both or neither) the stopping
    test, its arguments and ``info`` are those of ``lp_admm_batch_until``.

    A wrong shape, a NaN, an infinite entry of a batched ``beq`` or ``b_lower[k] > b_upper[k]`` on a row (both name the instance)
    raises ``ValueError`` before the library is loaded, like every error of ``lp_admm_batch`` and of the stopping arguments.
    """
    stop, rhs = _check_admm_batch_rhs_call(cs, a_eq, beq, a_ineq, b_lower, b_upper, tol_residual, tol_step, check_every)
    return _admm_batch_rhs_run(cs, a_eq, beq, a_ineq, rhs, lb, ub, stop, x0, gamma_eq, gamma_ineq, nb_iter, callback_func, max_time,
                               use_preconditioning, nb_iter_plot)


def _check_admm_batch_rhs_call(cs, a_eq, beq, a_ineq, b_lower, b_upper, tol_residual, tol_step, check_every):
    """What ``lp_admm_batch_rhs`` checks of its own, without the library: ``(stop, rhs)``, ``stop`` the checked ``(tol_residual,
    tol_step, check_every)`` or None, ``rhs`` the three sides as ``_check_batch_rhs`` returns them."""
    stop = None
    if tol_residual is not None or tol_step is not None:
        if tol_residual is None or tol_step is None:
            raise ValueError("tol_residual and tol_step go together: give both, or neither for the fixed horizon")
        tol_residual, check_every = _many.check_stop(tol_residual, check_every, "tol_residual")
        tol_step, _ = _many.check_stop(tol_step, check_every, "tol_step")
        stop = (tol_residual, tol_step, check_every)
    from .tools import CsrArrays

    if np.ndim(cs) != 2:
        raise ValueError(f"cs has shape {np.shape(cs)}: expected (B, n), one row of costs per instance")
    batch = np.shape(cs)[0]
    shapes = [0 if a is None else CsrArrays.from_any(a).shape[0] for a in (a_eq, a_ineq)]
    return stop, _check_batch_rhs(batch, shapes[0], shapes[1], beq, b_lower, b_upper)


def _admm_batch_rhs_run(cs, a_eq, beq, a_ineq, rhs, lb, ub, stop, x0, gamma_eq, gamma_ineq, nb_iter, callback_func, max_time,
                        use_preconditioning, nb_iter_plot):
    """``lp_admm_batch_rhs`` behind its checks (``_check_admm_batch_rhs_call`` gives ``stop`` and ``rhs``)."""
    first = [None if v is None else (v[0] if v.ndim == 2 else v) for v in rhs]   # the state is created with instance 0's sides
    if a_eq is not None and beq is None:
        raise ValueError("a_eq without beq")
    if a_eq is not None and first[0] is None:
        first[0] = beq
    rhs = tuple(v if v is not None and v.ndim == 2 else None for v in rhs)   # a 1-D side is the one the state is created with
    return _admm_batch_run(cs, a_eq, first[0], a_ineq, first[1], first[2], lb, ub, x0, gamma_eq, gamma_ineq, nb_iter, callback_func, max_time,
                           use_preconditioning, nb_iter_plot, stop, rhs=rhs if any(v is not None for v in rhs) else None)


# ---------------------------------------------------------------------------------------------------------------------
# a list of LPs with different matrices: one workgroup per LP
def _admm_many_problem(k, problem):
    """LP ``k`` of a list, validated (``ValueError``) without touching the library:
    ``(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub)`` with the matrices as ``CsrArrays`` (``a_eq``: ``None`` for an LP without
    equality rows) and the vectors as contiguous float64 arrays (``b_lower`` / ``b_upper``: -inf / +inf where absent)."""
    from .tools import CsrArrays

    c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub = _many.unpack_problem(k, problem)
    c = _many.check_cost(k, "c", c, finite=True)
    n = c.size
    lb, ub = (_many.check_vector(k, name, v, (n,), f"c has {n} entries", no_nan=True) for name, v in (("lb", lb), ("ub", ub)))
    a_eq, a_ineq = CsrArrays.from_any(a_eq), CsrArrays.from_any(a_ineq)
    if a_ineq is None:
        raise ValueError(f"LP {k} has no inequality block: the reference cannot form the standard form without one (tools.py:92)")
    if a_eq is not None and a_eq.shape[0] == 0:
        a_eq, beq = None, None
    for name, a in (("a_eq", a_eq), ("a_ineq", a_ineq)):
        if a is not None:
            _many.check_csr(k, name, a, n, f"c has {n} entries")

    def rhs(name, v, rows, fill):
        return np.full(rows, fill) if v is None else _many.check_vector(k, name, v, (rows,), f"expected ({rows},)", no_nan=True)

    if a_eq is not None:
        if beq is None:
            raise ValueError(f"LP {k}: a_eq without beq")
        beq = rhs("beq", beq, a_eq.shape[0], 0.0)
    b_lower = rhs("b_lower", b_lower, a_ineq.shape[0], -np.inf)
    b_upper = rhs("b_upper", b_upper, a_ineq.shape[0], np.inf)
    return c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub


def admm_many_system(lps):
    """The LPs ``(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub)`` of ``_admm_many_problem`` as the one block-diagonal LP
    ``slp_admm_many_create`` takes -- pure numpy, no library.  A dict of:

    ``n``, ``m_eq``, ``m_ineq``: the shapes, int64 arrays of length ``count``;
    ``col0``, ``eq0``, ``in0``: first column, first row of the equality block and first row of the inequality block of every LP;
    ``x0`` (``lam0``): where the LP's ``N_k = n_k + m_ineq,k`` standard-form unknowns (its ``m_k = m_eq,k + m_ineq,k`` multipliers)
    begin in the LP-by-LP vectors the solver returns;
    ``eq_indptr``, ``eq_indices``, ``eq_data``, ``b_eq``: the equality rows of all LPs (LP 0, LP 1, ...), the columns of LP k offset by
    ``col0[k]``; ``in_indptr``, ``in_indices``, ``in_data``, ``b_lower``, ``b_upper``: the same for the inequality rows;
    ``c``, ``lb``, ``ub`` concatenated LP by LP.

    The standard form of this composite has all original variables first and all slacks after them, which keeps the relative
    order of every LP's columns and rows: the set-up chain of ``lp_admm`` on the composite gives every LP the bits of its own."""
    n = np.array([lp[0].size for lp in lps], dtype=np.int64)
    m_eq = np.array([0 if lp[1] is None else lp[1].shape[0] for lp in lps], dtype=np.int64)
    m_ineq = np.array([lp[3].shape[0] for lp in lps], dtype=np.int64)
    if int(n.sum() + m_ineq.sum()) >= 2 ** 31 or int(m_eq.sum() + m_ineq.sum()) >= 2 ** 31:
        raise ValueError("the list has 2^31 or more variables + slacks or rows in total")
    col0 = first_offsets(n)
    out = dict(n=n, m_eq=m_eq, m_ineq=m_ineq, col0=col0, eq0=first_offsets(m_eq), in0=first_offsets(m_ineq),
               x0=first_offsets(n + m_ineq), lam0=first_offsets(m_eq + m_ineq))
    for tag, part, rhs_names in (("eq", 1, (("b_eq", 2),)), ("in", 3, (("b_lower", 4), ("b_upper", 5)))):
        have = [k for k, lp in enumerate(lps) if lp[part] is not None]
        out[tag + "_indptr"], out[tag + "_indices"], out[tag + "_data"] = _many.stack_blocks(
            [(lps[k][part].indptr, lps[k][part].indices, lps[k][part].data) for k in have], col0[have])
        for name, pos in rhs_names:
            out[name] = concat([lp[pos] for lp in lps if lp[part] is not None], np.float64)
    for name, pos in (("c", 0), ("lb", 6), ("ub", 7)):
        out[name] = concat([lp[pos] for lp in lps], np.float64)
    return out


def _admm_many_starts(x0, lps):
    """``x0`` of ``lp_admm_many`` checked against the LPs: ``None``, or a list with one start (or ``None``) per LP."""
    return _many.check_starts(x0, lps, finite=True)


def admm_many_lds_limit():
    """Doubles of x, y, lambda (``2 N + m``) an LP may hold in LDS (``slp_admm_many_lds_limit``)."""
    return int(_lib.load().slp_admm_many_lds_limit())


class ADMMManyState(_many.ManyState):
    """Device-resident ADMM state of a list of LPs (thin RAII wrapper of ``slp_admm_many``).  ``lps``: the LPs as
    ``_admm_many_problem`` returns them; ``x0``: ``None`` or one start (or ``None``: zeros) per LP, as ``_admm_many_starts``
    returns it."""

    _PREFIX = "slp_admm_many"
    _LIVE = "slp_many_admm"

    def __init__(self, lps, x0=None, gamma_eq=2, gamma_ineq=3, use_preconditioning=True):
        if len(lps) < 1:
            raise ValueError("an empty list of LPs")
        s = admm_many_system(lps)
        self.count = len(lps)
        self.n, self.N, self.m = s["n"], s["n"] + s["m_ineq"], s["m_eq"] + s["m_ineq"]
        self.system = s
        start = _many.concat_starts(x0, self.n)
        has_eq = int(s["m_eq"].sum()) > 0
        eq = tuple(_lib.ptr(s[name]) if has_eq else None for name in ("eq_indptr", "eq_indices", "eq_data", "b_eq"))
        # all of the above needs no GPU; the library is loaded (and bound to a device) only now
        self._l = _lib.lib()
        self._h = _lib.check_handle(self._l.slp_admm_many_create(
            self.count, _lib.ptr(s["n"]), _lib.ptr(s["m_eq"]), _lib.ptr(s["m_ineq"]), *eq, _lib.ptr(s["in_indptr"]),
            _lib.ptr(s["in_indices"]), _lib.ptr(s["in_data"]), _lib.ptr(s["b_lower"]), _lib.ptr(s["b_upper"]), _lib.ptr(s["c"]),
            _lib.ptr(s["lb"]), _lib.ptr(s["ub"]), _lib.ptr(start), float(gamma_eq), float(gamma_ineq), int(bool(use_preconditioning))))

    def iterate(self, k):
        _lib.check(self._l.slp_admm_many_iterate(self._h, int(k)))

    def sweep_step(self):
        _lib.check(self._l.slp_admm_many_sweep_step(self._h))

    def multiplier_step(self):
        _lib.check(self._l.slp_admm_many_multiplier_step(self._h))

    def report(self):
        """``(count, 3)``: augmented-Lagrangian energy, max |A x - b|, max(0, -min x) per LP."""
        out = np.zeros((self.count, 3))
        _lib.check(self._l.slp_admm_many_report(self._h, _lib.ptr(out)))
        return out

    def set_stop(self, tol_residual, tol_step, check_every=1):
        """Arms the per-LP stopping test of the iteration kernel (``slp_many_admm_set_stop``): at the end of every iteration ``t``
        of an LP with ``t % check_every == 0`` -- counted from 1 over the LP's life; an iteration is the right-hand side, the sweep
        and the multiplier update -- the LP stops iff ``max|A x_t - b| <= tol_residual`` (the rows of its standard form) and
        ``max|x_t - x_{t-1}| <= tol_step`` (all ``N`` columns, slacks included); a stopped LP keeps its iterate and takes no part in
        later calls.  ``tol_residual=None`` turns the test off, the state after the constructor.  Between whole iterations only
        (not between ``sweep_step`` and ``multiplier_step``).  Every call clears the stopped flags and keeps the counters."""
        if tol_residual is None:
            tol_residual, tol_step, check_every = -1.0, 0.0, 1
        else:
            tol_residual, check_every = _many.check_stop(tol_residual, check_every, "tol_residual")
            tol_step, _ = _many.check_stop(tol_step, check_every, "tol_step")
        _lib.check(self._l.slp_many_admm_set_stop(self._h, tol_residual, tol_step, check_every))

    def stop_state(self):
        """``(iterations, stopped, residual, step)`` per LP, int64, bool and two float64 arrays: the iterations completed (for a
        stopped LP its stopping iteration), whether it is stopped and the last evaluated residual and step (``+inf`` before the
        first test)."""
        iterations, stopped = np.zeros(self.count, dtype=np.int64), np.zeros(self.count, dtype=np.int32)
        residual, step = np.zeros(self.count), np.zeros(self.count)
        _lib.check(self._l.slp_many_admm_stop_state(self._h, _lib.ptr(iterations), _lib.ptr(stopped), _lib.ptr(residual), _lib.ptr(step)))
        return iterations, stopped.astype(bool), residual, step

    def x(self, full=False):
        """Per LP the first ``n_k`` entries of its iterate, or with ``full`` all ``N_k`` of its standard form."""
        return self._per_lp("x", self.N if full else self.n, int(bool(full)))

    def lam(self):
        """Per LP ``[lambda_eq; lambda_ineq]``."""
        return self._per_lp("lambda", self.m)

    def num_levels(self, k):
        """Dependency levels of LP ``k``'s sweep: those of the plan of that LP alone."""
        return int(self._l.slp_admm_many_num_levels(self._h, self._of_lp(k)))

    def kmax(self, form):
        """Iterations one launch of the form (``"lds"`` / ``"global"``) holds; 0 when no LP runs in it."""
        return int(self._l.slp_admm_many_kmax(self._h, self.FORMS.index(form)))

    def bench(self, k):
        """GPU milliseconds per iteration of the whole list over ``k`` iterations (HIP events)."""
        ms = np.zeros(1)
        _lib.check(self._l.slp_admm_many_bench(self._h, int(k), _lib.ptr(ms)))
        return float(ms[0])


def lp_admm_many(
    problems,
    x0=None,
    gamma_eq=2,
    gamma_ineq=3,
    nb_iter=100,
    callback_func=None,
    max_time=None,
    use_preconditioning=True,
    nb_iter_plot=10,
):
    """``lp_admm`` for a list of LPs whose matrices differ (extension; the reference solves one LP per call).

    ``problems`` is a sequence of 8-tuples ``(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub)``, each as ``lp_admm`` takes them
    (``a_eq`` may be ``None`` or a matrix without rows; the inequality block is required, tools.py:92); ``x0`` is ``None`` or a
    sequence with one start (or ``None``) per LP; ``gamma_eq``, ``gamma_ineq`` and ``use_preconditioning`` are shared.  Every shape,
    finiteness and column-index error is a ``ValueError`` that names the LP, raised before the library is loaded.  The LPs become
    one block-diagonal LP whose set-up chain (ADMM.py:73-101) runs once on the device; every LP is then one workgroup that runs
    whole iterations inside one launch, its iterates in LDS where they fit (pysparselp_amd/csrc/slp_admm_many.hip); every LP is
    bit for bit what ``lp_admm(..., order=ORDER_SEQUENTIAL)`` computes for it alone.

    The loop is that of ``lp_admm``: ``nb_iter + 1`` sweeps, a report after those with ``i % nb_iter_plot == 0`` --
    ``callback_func(i, xs, energy, energy, elapsed, max_violated_equality, max_violated_inequality)`` with ``xs`` a list of
    arrays and the rest arrays of length ``count``; ``max_time`` stops the whole list at a report.  Returns the list of ``x``.

    Under a communicator every rank solves the whole list (a replica).  For LPs that share one matrix ``lp_admm_batch`` builds
    ``M`` and its plan once for all of them.
    """
    xs, _ = _admm_many_run(problems, x0, gamma_eq, gamma_ineq, nb_iter, callback_func, max_time, use_preconditioning, nb_iter_plot, None)
    return xs


def _admm_many_run(problems, x0, gamma_eq, gamma_ineq, nb_iter, callback_func, max_time, use_preconditioning, nb_iter_plot, stop):
    """``lp_admm_many`` (``stop`` None) and ``lp_admm_many_until`` (``stop`` the checked ``(tol_residual, tol_step,
    check_every)``): ``(xs, info)``, ``info`` None without a stopping test."""
    count = _many.count_problems(problems)
    lps = [_admm_many_problem(k, p) for k, p in enumerate(problems)]
    x0 = _admm_many_starts(x0, lps)
    solved = np.arange(count)  # every LP has an inequality block: all take part
    info = None if stop is None else _many.new_stop_info(count, solved, residual=True)
    state = ADMMManyState(lps, x0, gamma_eq, gamma_ineq, use_preconditioning)

    def stopped_now():
        now = state.stop_state()
        _many.spread_stop_state(info, solved, now)
        return now[1]

    try:
        if stop is not None:
            state.set_stop(*stop)
            if callback_func is not None:
                try:
                    callback_func.info = info
                except AttributeError:   # a bound method takes no attribute: wrap it in a function to read ``info``
                    pass
        start = time.perf_counter()
        i = 0
        while i <= nb_iter:  # ADMM.py:143: nb_iter + 1 sweeps
            if i % nb_iter_plot == 0:
                if stop is not None and stopped_now().all():
                    break
                state.sweep_step()
                elapsed = time.perf_counter() - start
                if max_time is not None and elapsed > max_time:
                    break
                energy, max_violated_equality, max_violated_inequality = state.report().T.copy()
                if callback_func is not None:
                    callback_func(i, state.x(), energy, energy.copy(), elapsed, max_violated_equality, max_violated_inequality)
                state.multiplier_step()
                i += 1
            else:
                k = min(nb_iter_plot - i % nb_iter_plot, nb_iter + 1 - i)
                state.iterate(k)
                i += k
        if stop is not None:
            stopped_now()
        return state.x(), info
    finally:
        state.close()


def lp_admm_many_until(
    problems,
    tol_residual,
    tol_step,
    check_every=10,
    x0=None,
    gamma_eq=2,
    gamma_ineq=3,
    nb_iter=10000,
    callback_func=None,
    max_time=None,
    use_preconditioning=True,
    nb_iter_plot=10,
):
    """``lp_admm_many`` with a stopping test per LP (extension; the reference has no stopping test): the list runs until every LP
    has stopped, at most ``nb_iter + 1`` sweeps.  Returns ``(xs, info)``.

    The test is made inside the iteration kernel (``ADMMManyState.set_stop``), at the end of every iteration ``t`` of an LP with
    ``t % check_every == 0``, iterations counted from 1 (an iteration is the right-hand side, the sweep that gives ``x_t`` and the
    multiplier update that gives ``lambda_t``): the LP stops iff ``max|A x_t - b| <= tol_residual``, over the rows of its standard
    form and with the very residual the multiplier update forms, and ``max|x_t - x_{t-1}| <= tol_step``, over all ``n + m_ineq``
    columns of the standard form; a NaN in either never stops.  A stopped LP keeps ``x_t`` and ``lambda_t``, bit for bit those of
    ``lp_admm(..., nb_iter=t - 1, order=ORDER_SEQUENTIAL)``, while the others go on.  ``tol_residual`` and ``tol_step`` are
    finite floats ``>= 0``, ``check_every`` an int ``>= 1``: a ``ValueError`` that names the argument, before the library is
    loaded, otherwise, like every shape error.

    ``info`` is a dict of arrays over the list: ``iterations`` (int64: completed, for a stopped LP its stopping iteration),
    ``stopped`` (bool), ``residual`` and ``step`` (float64: the last evaluated ones, ``+inf`` before the first test).

    The loop and the cadence of reports are those of ``lp_admm_many``: a report at index ``i`` lies between sweep ``i + 1`` and its
    multiplier update.  The loop ends at the first report index at which every LP is stopped (no callback for that index), at
    ``nb_iter``, or at ``max_time``.  In a callback a stopped LP's ``xs[k]`` is its final iterate and its three numbers are the
    report on that frozen state, so its ``max_violated_equality`` equals ``info["residual"][k]`` exactly.  ``info`` is current at
    every callback: the same dict, updated in place, is set as the ATTRIBUTE ``callback_func.info`` before the first call (a
    function or any object that takes attributes; a bound method takes none and has to be wrapped in a function to read it).
    """
    tol_residual, check_every = _many.check_stop(tol_residual, check_every, "tol_residual")
    tol_step, _ = _many.check_stop(tol_step, check_every, "tol_step")
    return _admm_many_run(problems, x0, gamma_eq, gamma_ineq, nb_iter, callback_func, max_time, use_preconditioning, nb_iter_plot,
                          (tol_residual, tol_step, check_every))


def lp_admm2(
    c,
    a_eq,
    beq,
    a_ineq,
    b_lower,
    b_upper,
    lb,
    ub,
    x0=None,
    gamma_ineq=0.7,
    nb_iter=100,
    callback_func=None,
    max_time=None,
    use_preconditioning=False,
    nb_iter_plot=10,
    cg_tol=1e-13,
    cg_max_steps=500,
):
    """minimise c.x  s.t.  a_eq x = beq,  b_lower <= a_ineq x <= b_upper,  lb <= x <= ub  (reference ADMM.py:272-474).

    ADMM with the equality constraints of the slack standard form kept exact in every x-step.  Where the reference factorises
    the KKT matrix ``[gamma I, A^T; A, 0]`` once with a sparse LU (:330-342), the x-step here is the matrix-free projection of
    csrc/slp_blocks.hip (conjugate gradients on the device, relative residual ``cg_tol``, at most ``cg_max_steps`` steps,
    warm-started): the iterates agree with the LU form to that tolerance, not bit for bit.  Same signature, reporting cadence
    (``nb_iter + 1`` iterations, a report after those with ``niter % nb_iter_plot == 0``, ``max_time`` checked there before
    the callback) and return value (the first ``n`` entries of the over-relaxed ``x``, :474).  ``max_time=None`` means no
    limit.  ``[A_eq; A_ineq]`` is uploaded as the caller holds it (row chunks when it would not fit the device); the slack
    column stays implicit.  ``use_preconditioning=True`` runs the reference's transforms (:308-330) on the host and hands
    the explicit standard form over, all rows equalities (not for LPs that need chunks)."""
    from . import host_setup
    from .scale import DeviceADMM2
    from .tools import CsrArrays

    start = time.perf_counter()
    c = _lib.f64(c)
    n = c.size
    a_eq, a_ineq = CsrArrays.from_any(a_eq), CsrArrays.from_any(a_ineq)
    if a_ineq is None:  # what the reference does on this input (tools.py:92-127)
        raise UnboundLocalError("local variable 'a_eq2' referenced before assignment (no inequality constraints)")
    x0 = np.zeros(n) if x0 is None else _lib.f64(x0)
    if use_preconditioning:  # :308-318, :320-322, :328-329
        if a_eq is not None:
            a_eq, beq = precondition_constraints(a_eq, beq, alpha=2)
        a_ineq, b_lower, b_upper = precondition_constraints(a_ineq, b_lower, b_upper, alpha=2)
        c, a, b, lb, ub, x0 = convert_to_standard_form_with_bounds(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0)
        a, b = precondition_constraints(a, b, alpha=2)
        if host_setup.chunk_entries(a.nnz, a.shape[0], a.shape[1]) is not None:
            raise ValueError("lp_admm2 with use_preconditioning=True needs the explicit standard form in one piece, and this LP "
                             "would be built from row chunks; " + host_setup.MULTI_GPU)
        eq, ineq, m_eq, b_all, bl_all = a, None, a.shape[0], _lib.f64(b), None
    else:
        m_eq = 0 if a_eq is None else a_eq.shape[0]
        m_in = a_ineq.shape[0]
        b_upper = np.full(m_in, np.inf) if b_upper is None else _lib.f64(b_upper)
        b_lower = np.full(m_in, -np.inf) if b_lower is None else _lib.f64(b_lower)
        b_all = np.concatenate((np.zeros(0) if a_eq is None else _lib.f64(beq), b_upper))
        bl_all = np.concatenate((np.zeros(m_eq), b_lower))
        eq, ineq = a_eq, a_ineq
    ncol = ineq.shape[1] if ineq is not None else eq.shape[1]
    nrow = (0 if eq is None else eq.shape[0]) + (0 if ineq is None else ineq.shape[0])
    entries = host_setup.chunk_entries(host_setup.nnz_of(eq, ineq), nrow, ncol)
    mat, _ = host_setup.upload(eq, ineq, ncol, entries)
    state = None
    try:
        state = DeviceADMM2(mat, b_all, c, lb, ub, m_eq=m_eq, b_lower=bl_all, x0=x0, gamma=gamma_ineq, cg_tol=cg_tol,
                            cg_max_steps=cg_max_steps)
        i = 0
        while i <= nb_iter:  # :407: nb_iter + 1 iterations, a report after those with i % nb_iter_plot == 0
            k = 1 if i % nb_iter_plot == 0 else min(nb_iter_plot - i % nb_iter_plot, nb_iter + 1 - i)
            reports = (i + k - 1) % nb_iter_plot == 0
            state.iterate(k)
            i += k
            if reports:
                elapsed = time.perf_counter() - start
                if max_time is not None and elapsed > max_time:
                    break
                energy = state.report()[0]
                if callback_func is not None:
                    callback_func(i - 1, state.x(n), energy, energy, elapsed, 0, 0)
        return state.x(n)
    finally:
        if state is not None:
            state.close()
        mat.close()
