"""Gradient ascent in the dual with an exact line search, on the GPU (reference DualGradientAscent.py:36-245).

The dual function of ``min c.x, A_e x = b_e, A_i x <= b_u, lb <= x <= ub`` is concave and piecewise linear in the multipliers;
every iteration moves the inequality multipliers, then the equality multipliers, along their (masked) gradient to the exact
maximiser on that line -- a sort of the breakpoints ``-c_bar_j / d_j``, two running sums and a bisection
(csrc/slp_dga.hip).  The multipliers it returns are dual feasible, so their dual energy (``DeviceDGA.report``) is a certified
lower bound on the LP's value.  ``DeviceDGABatch`` / ``dual_gradient_ascent_batch`` advance B LPs that share the constraint
matrix and the right-hand sides together (csrc/slp_dga_batch.hip); instance k is bit for bit the single solve of its data.
``DeviceDGAMany`` / ``dual_gradient_ascent_many`` advance a list of LPs with matrices of their own, one workgroup per LP and whole
iterations inside a launch (csrc/slp_dga_many.hip); LP k is bit for bit the single solve of ``lps[k]``.
``DeviceDGAMany.set_stop`` / ``dual_gradient_ascent_many_until`` stop every LP of such a list on its own, by a test on the step of
its multipliers inside the iteration kernel; ``DeviceDGAMany.set_cutoff`` / ``dual_gradient_ascent_many_cutoff`` also once its
certified lower bound has reached a cut-off, evaluated in the same kernel; ``DeviceDGAMany.set_compaction`` /
``dual_gradient_ascent_many_compact`` hand the LPs still moving consecutive workgroups in every launch.  ``DeviceDGABatch.set_stop`` / ``dual_gradient_ascent_batch_until`` stop every instance
of a batch on its own, on that step or once its certified lower bound has reached a cut-off, tested on the device.
"""
import os
import time

import numpy as np

from . import _lib
from . import _many
from ._batch import check_costs, check_rhs, check_targets, concat, first_offsets, require_one_sided, shared_or_batched, split_by

PATHS = {"auto": 0, "fused": 1, "general": 2}
FUSED_MAX = 8192    # most variables of the fused search (one workgroup, breakpoints in LDS)
FUSED_AUTO = 2048   # ... and up to where it is the default (beyond, the general search is faster)
FUSED_BATCH = 32    # batched: from this many instances on the fused search is the default up to FUSED_MAX variables
STATUS_NEGATIVE_STEP, STATUS_EMPTY, STATUS_DRAWS_DRY, STATUS_NAN, STATUS_NO_CROSSING = 1, 2, 4, 8, 16


def _check_status(flags):
    if flags & STATUS_NAN:
        raise ValueError("dual gradient ascent: a breakpoint or a step is NaN (an infinite bound meets a zero reduced cost or an "
                         "infinite direction): outside what the method is defined for")
    if flags & STATUS_EMPTY:
        raise ValueError("exact_dual_line_search: the direction meets no column (empty breakpoint set)")
    if flags & STATUS_NO_CROSSING:
        raise ValueError("exact_dual_line_search: the derivative never changes sign (the dual is unbounded along the direction)")
    if flags & STATUS_NEGATIVE_STEP:
        raise AssertionError("exact_dual_line_search returned a negative step")


def _check_status_each(flags, where):
    """The single solver's exception for the first kind of error present, naming the readers that carry it: ``where`` is
    ``"instances {} of the batch"`` or ``"LPs {} of the list"``."""
    flags = np.asarray(flags, dtype=np.int64)
    for bit in (STATUS_NAN, STATUS_EMPTY, STATUS_NO_CROSSING, STATUS_NEGATIVE_STEP):
        bad = np.flatnonzero(flags & bit)
        if bad.size:
            try:
                _check_status(bit)
            except (ValueError, AssertionError) as e:
                raise type(e)(f"{e} ({where.format(bad.tolist())})") from None


def _check_status_batch(flags):
    _check_status_each(flags, DeviceDGABatch._WHERE)


class _DeviceDGA:
    """What the three device wrappers share: the handle ``_h`` of the entry points ``slp_<_PREFIX>_*`` and ``_draws``, the
    callable that continues the stream of tie draws.  ``_WHERE`` names the readers of a status error (None: one solve)."""

    _PREFIX = None
    _WHERE = None

    def _call(self, name, *args):
        return getattr(self._l, f"slp_{self._PREFIX}_{name}")(self._h, *args)

    def close(self):
        if getattr(self, "_h", None):
            self._call("destroy")
            self._h = None

    __del__ = close

    def push_random(self, values):
        values = _lib.f64(values)
        _lib.check(self._call("push_random", _lib.ptr(values), values.size))

    def iterate(self, k, refill=True):
        """``k`` iterations (of every instance / LP), nothing read back in between.  ``refill``: the draw buffer is topped up to
        two draws per iteration behind the furthest reader first; without it the call stops early, for all readers, when the
        buffer could run dry (``status()[3]`` tells how far it got)."""
        k = int(k)
        if refill:
            left = self.status()[2]
            if left < 2 * k:
                self.push_random(self._draws(2 * k - left))
        _lib.check(self._call("iterate", k))

    def check(self):
        flags = self.status()[0]
        if self._WHERE is None:
            _check_status(flags & ~STATUS_DRAWS_DRY)
        else:
            _check_status_each(flags & ~STATUS_DRAWS_DRY, self._WHERE)
        return flags

    def timing(self, on):
        _lib.check(self._call("timing", int(bool(on))))

    def timing_read(self):
        """Milliseconds per stage since ``timing(True)``: products, sort, scans, rest, fused search (the list form runs an
        iteration as one launch, so all of it stands under ``fused_search``)."""
        out = np.zeros(5)
        _lib.check(self._call("timing_read", _lib.ptr(out)))
        return dict(zip(("products", "sort", "scans", "rest", "fused_search"), (float(v) for v in out)))


class DeviceDGA(_DeviceDGA):
    """The iteration state on the device (``slp_dga_*``): ``a`` a ``DeviceMatrix`` (any product format, chunked included) whose
    first ``m_eq`` rows are the equalities, ``b`` = ``[b_eq; b_upper]``, ``y0`` the start multipliers, ``draws`` a callable
    ``draws(count)`` giving the next ``count`` uniform draws of the tie rule (default: a private ``RandomState(0)``).
    ``path``: ``"auto"`` (the fused one-workgroup search up to ``FUSED_AUTO`` variables, else the general one), ``"fused"``
    (at most ``FUSED_MAX`` variables), ``"general"``; the environment's ``SLP_DGA_PATH`` picks it when ``path`` is None."""

    _PREFIX = "dga"

    def __init__(self, a, b, c, lb, ub, y0, m_eq=0, draws=None, path=None):
        self._l = _lib.lib()
        self.n, self.m, self.m_eq = a.shape[1], a.shape[0], int(m_eq)
        assert 0 <= self.m_eq <= self.m
        b, c, lb, ub, y0 = _lib.f64(b), _lib.f64(c), _lib.f64(lb), _lib.f64(ub), _lib.f64(y0)
        assert b.size == self.m and y0.size == self.m and c.size == self.n and lb.size == self.n and ub.size == self.n
        self._draws = draws if draws is not None else np.random.RandomState(0).random_sample
        self._h = _lib.check_handle(self._l.slp_dga_create_on(a._h, self.m_eq, _lib.ptr(b), _lib.ptr(c), _lib.ptr(lb), _lib.ptr(ub),
                                                              _lib.ptr(y0)))
        self._a = a
        if path is not None:
            _lib.check(self._l.slp_dga_set_path(self._h, PATHS[path]))

    def path(self):
        return {1: "fused", 2: "general"}[int(self._l.slp_dga_path(self._h))]

    def status(self):
        """``(flags, tie draws taken, draws left in the buffer, iterations done)``; reading it synchronises."""
        out = np.zeros(4, dtype=np.int64)
        _lib.check(self._l.slp_dga_status(self._h, _lib.ptr(out)))
        return tuple(int(v) for v in out)

    def x(self):
        x = np.empty(self.n)
        _lib.check(self._l.slp_dga_get_x(self._h, _lib.ptr(x)))
        return x

    def y(self):
        y = np.empty(self.m)
        _lib.check(self._l.slp_dga_get_y(self._h, _lib.ptr(y)))
        return y[:self.m_eq].copy(), y[self.m_eq:].copy()

    def report(self):
        """``(dual energy, largest violation, sum of violations)`` of the multipliers as they are, x their dual argmin."""
        out = np.zeros(3)
        _lib.check(self._l.slp_dga_report(self._h, _lib.ptr(out)))
        return tuple(float(v) for v in out)


def exact_dual_line_search(direction, a, b, c_bar, upper_bounds, lower_bounds, draws=None, path=None):
    """The step along ``direction`` that maximises the dual (reference :36-65), on the device (``slp_dga_line_search``).
    ``direction``: the reference's 1 x m sparse row, or m dense values; ``a``: scipy CSR of the m rows.  A tie takes its uniform
    draw from ``draws`` (a sequence) or, as the reference does, from ``numpy.random.rand()`` -- only when a tie occurs."""
    import scipy.sparse

    from .device import DeviceMatrix

    if scipy.sparse.issparse(direction):
        direction = direction.toarray()
    g = np.asarray(direction, dtype=np.float64).ravel()
    g, b, c_bar = _lib.f64(g), _lib.f64(b), _lib.f64(c_bar)
    ub, lb = _lib.f64(upper_bounds), _lib.f64(lower_bounds)
    a = a.tocsr() if scipy.sparse.issparse(a) else a
    assert g.size == a.shape[0] == b.size and c_bar.size == a.shape[1] == ub.size == lb.size
    if path is None:
        path = os.environ.get("SLP_DGA_PATH", "auto")
    mat = DeviceMatrix.from_csr(a)
    try:
        given = _lib.f64(np.zeros(0) if draws is None else draws)
        while True:
            out = np.zeros(4)
            _lib.check(mat._l.slp_dga_line_search(mat._h, _lib.ptr(g), _lib.ptr(b), _lib.ptr(c_bar), _lib.ptr(ub), _lib.ptr(lb),
                                                  PATHS[path], _lib.ptr(given), given.size, _lib.ptr(out)))
            flags = int(out[1])
            if flags & STATUS_DRAWS_DRY and draws is None and given.size == 0:
                given = _lib.f64([np.random.rand()])   # a tie: the reference's draw, and the search again with it
                continue
            break
    finally:
        mat.close()
    if flags & STATUS_DRAWS_DRY:
        raise ValueError("exact_dual_line_search: a tie and no draw left in `draws`")
    _check_status(flags & ~STATUS_NEGATIVE_STEP)
    return float(out[0])


def _dga_drive(state, nb_max_iter, callback_func, max_time, start, all_frozen=False, all_still=None):
    """The loop of the three forms: iteration ``niter`` with ``niter % 100 == 0`` is a launch of its own, followed by the status
    check, the callback with the x of the top of that iteration and the test of ``max_time``; the iterations between two such
    are one call.  Nothing runs when every reader is frozen.  ``all_still()`` (a list with a stopping test), asked after every
    call and before its callback: true once no LP moves any more, which ends the loop behind that callback."""
    i = 0
    while i < nb_max_iter and not all_frozen:
        k = 1 if i % 100 == 0 else min(100 - i % 100, nb_max_iter - i)
        state.iterate(k)
        i += k
        state.check()
        still = all_still is not None and all_still()
        if (i - 1) % 100 == 0:
            elapsed = time.perf_counter() - start
            if callback_func is not None:
                callback_func(i - 1, state.x(), 0, 0, elapsed, 0, 0)
            if max_time is not None and elapsed > max_time:
                break
        if still:
            break


def dual_gradient_ascent(x, lp, nb_max_iter=1000, callback_func=None, y_eq=None, y_ineq=None, max_time=None, nb_iter_plot=1):
    """Gradient ascent in the dual (reference :68-245), same signature and return value ``(x, y_eq, y_ineq)``.

    ``lp``: any object with the reference's attributes (``costsvector, a_equalities, b_equalities, a_inequalities, b_upper,
    b_lower, lower_bounds, upper_bounds``); a finite ``b_lower`` is refused with ``ValueError`` (the reference's assert, :82)
    before anything is uploaded.  The start is the reference's: ``y_eq = -rand(m_eq)``, ``y_ineq = |rand(m_ineq)|`` from seed 0,
    and the tie draws of the line search continue that stream -- from a private ``RandomState(0)``; numpy's global generator
    is left alone.  A dual-infeasible start (energy ``-inf``) returns at once, as in the reference (:136-139).
    ``callback_func(niter, x, 0, 0, elapsed, 0, 0)`` is called for ``niter % 100 == 0`` with the x of the top of that iteration;
    ``nb_iter_plot`` only gates the reference's prints and is unused.  ``max_time``, which the reference tests after every
    iteration, is tested where the device loop synchronises anyway: after those callbacks, so at most every 100 iterations;
    the points of a curve do not depend on it.  Under a communicator every rank runs the whole LP as a replica."""
    require_one_sided(getattr(lp, "b_lower", None))
    from . import host_setup
    from .tools import CsrArrays

    start = time.perf_counter()
    c = _lib.f64(lp.costsvector)
    n = c.size
    a_eq, a_ineq = CsrArrays.from_any(lp.a_equalities), CsrArrays.from_any(lp.a_inequalities)
    m_eq = 0 if a_eq is None else a_eq.shape[0]
    m_in = 0 if a_ineq is None else a_ineq.shape[0]
    rs = np.random.RandomState(0)
    y_eq = -rs.rand(m_eq) if y_eq is None else _lib.f64(y_eq).copy()
    if y_ineq is None:
        y_ineq = np.abs(rs.rand(m_in)) if a_ineq is not None else None
    else:
        y_ineq = _lib.f64(y_ineq).copy()
    b = np.concatenate((_lib.f64(lp.b_equalities) if m_eq else np.zeros(0), _lib.f64(lp.b_upper) if m_in else np.zeros(0)))
    y0 = np.concatenate((y_eq, y_ineq if m_in else np.zeros(0)))
    eq, ineq = (a_eq if m_eq else None), (a_ineq if m_in else None)
    if eq is None and ineq is None:
        raise ValueError("dual_gradient_ascent: the LP has no constraint rows")
    entries = host_setup.chunk_entries(host_setup.nnz_of(eq, ineq), m_eq + m_in, n)
    mat, _ = host_setup.upload(eq, ineq, n, entries)
    state = None

    def result(xv):
        ye, yi = state.y()
        return xv, ye, (yi if a_ineq is not None else None)

    try:
        state = DeviceDGA(mat, b, c, lp.lower_bounds, lp.upper_bounds, y0, m_eq=m_eq, draws=rs.random_sample)
        if state.report()[0] == -np.inf:   # initial dual point not feasible (:133-139)
            return result(state.x())
        if nb_max_iter <= 0:
            return result(x)
        _dga_drive(state, nb_max_iter, callback_func, max_time, start)
        return result(state.x())
    finally:
        if state is not None:
            state.close()
        mat.close()


# ---- batched: B LPs over one constraint matrix ---------------------------------------------------------------------------------

class DeviceDGABatch(_DeviceDGA):
    """``DeviceDGA`` for B LPs over one ``DeviceMatrix`` ``a`` (with its CSR: not chunked) and one ``b`` (``slp_batch_dga_*``):
    ``c`` of shape ``(B, n)``; ``lb``, ``ub`` of shape ``(n,)`` or ``(B, n)``; ``y0`` of shape ``(m,)`` or ``(B, m)``; ``set_rhs``
    gives every instance a ``b`` of its own before the first iteration.  Results
    carry a leading axis B.  All instances read one stream of tie draws (``draws(count)``, default a private ``RandomState(0)``),
    each at its own position.  An instance whose start has dual energy ``-inf`` is frozen (``frozen()``): its x and y stay the
    start's.  ``path``: ``"auto"`` (the fused search, one workgroup per instance, up to ``FUSED_AUTO`` variables and, from
    ``FUSED_BATCH`` instances on, up to ``FUSED_MAX``; else the general one), ``"fused"``, ``"general"``; the environment's
    ``SLP_DGA_BATCH_PATH`` picks it when ``path`` is None."""

    _PREFIX = "batch_dga"
    _WHERE = "instances {} of the batch"

    def __init__(self, a, b, c, lb, ub, y0, m_eq=0, draws=None, path=None):
        self.n, self.m, self.m_eq = a.shape[1], a.shape[0], int(m_eq)
        c, self.batch = check_costs(c, self.n)
        if self.m < 1:
            raise ValueError("dual_gradient_ascent_batch: the LP has no constraint rows")
        if not 0 <= self.m_eq <= self.m:
            raise ValueError("m_eq out of range")
        c, b = _lib.f64(c), _lib.f64(b)
        if b.shape != (self.m,):
            raise ValueError(f"b has shape {b.shape}: expected ({self.m},); per-instance right-hand sides are not built")
        lb, lb_b = shared_or_batched("lower_bounds", lb, self.batch, self.n)
        ub, ub_b = shared_or_batched("upper_bounds", ub, self.batch, self.n)
        y0, y_b = shared_or_batched("y0", y0, self.batch, self.m)
        self._l = _lib.lib()
        self._draws = draws if draws is not None else np.random.RandomState(0).random_sample
        self._h = _lib.check_handle(self._l.slp_batch_dga_create_on(a._h, self.m_eq, _lib.ptr(b), self.batch, _lib.ptr(c), _lib.ptr(lb),
                                                                    int(lb_b), _lib.ptr(ub), int(ub_b), _lib.ptr(y0), int(y_b)))
        self._a = a
        if path is not None:
            _lib.check(self._l.slp_batch_dga_set_path(self._h, PATHS[path]))

    def path(self):
        return {1: "fused", 2: "general"}[int(self._l.slp_batch_dga_path(self._h))]

    def sort(self):
        """The sort of the general search: ``"segmented"`` or ``"global"`` (two device-wide stable sorts; the default for more than
        ``FUSED_AUTO`` variables, ``SLP_DGA_BATCH_SORT`` forces one); None on the fused path.  Same order, same bits."""
        return {0: None, 1: "segmented", 2: "global"}[int(self._l.slp_batch_dga_sort(self._h))]

    def status(self):
        """``(flags[B], tie draws taken[B], draws left in the buffer behind the furthest instance, iterations done)``; reading it
        synchronises."""
        out = np.zeros(2 * self.batch + 2, dtype=np.int64)
        _lib.check(self._l.slp_batch_dga_status(self._h, _lib.ptr(out)))
        per = out[:2 * self.batch].reshape(self.batch, 2)
        return per[:, 0].copy(), per[:, 1].copy(), int(out[-2]), int(out[-1])

    def frozen(self):
        out = np.zeros(self.batch, dtype=np.int32)
        _lib.check(self._l.slp_batch_dga_frozen(self._h, _lib.ptr(out)))
        return out.astype(bool)

    def x(self):
        x = np.empty((self.batch, self.n))
        _lib.check(self._l.slp_batch_dga_get_x(self._h, _lib.ptr(x)))
        return x

    def y(self):
        y = np.empty((self.batch, self.m))
        _lib.check(self._l.slp_batch_dga_get_y(self._h, _lib.ptr(y)))
        return y[:, :self.m_eq].copy(), y[:, self.m_eq:].copy()

    def report(self):
        """Array of shape ``(B, 3)``: per instance ``(dual energy, largest violation, sum of violations)`` of its multipliers as
        they are, x their dual argmin.  Column 0 is a certified lower bound on the instance's LP value."""
        out = np.zeros((self.batch, 3))
        _lib.check(self._l.slp_batch_dga_report(self._h, _lib.ptr(out)))
        return out

    def set_rhs(self, b):
        """Replaces the right-hand side (``slp_batch_dga_set_rhs``): ``b`` of shape ``(m,)`` -- one for all instances -- or ``(B, m)``
        over the rows of ``[A_eq; A_ineq]``, one row per instance.  Instance k is then bit for bit ``DeviceDGA`` on ``b[k]``: the
        gradient, ``g . b`` and the ``y . b`` of the energy read the instance's own vector, and which instances are frozen is
        derived again.  Only before the first iteration (``SlpError`` afterwards, the state keeps running with the right-hand
        sides it had); may be called more than once.  A wrong shape, a NaN, or an infinite entry of a batched ``b`` (the message
        names the instance) is a ``ValueError`` before the library is touched."""
        b, batched = check_rhs("b", b, self.batch, self.m, finite=True)
        _lib.check(self._l.slp_batch_dga_set_rhs(self._h, _lib.ptr(b), int(batched)))

    def set_stop(self, tol, targets=None, check_every=1):
        """Arms the per-instance stopping test (``slp_batch_dga_set_stop``): at the end of every iteration ``t`` with
        ``t % check_every == 0`` -- counted from 1 over the life of the state, the same number for every instance that moves -- an
        instance that is neither frozen nor stopped stops iff ``max|y_t - y_{t-1}| <= tol`` over all its multipliers (the
        inequality part after its clamp; a kind of rows that does not move contributes 0) or its dual energy, bit for bit
        ``report()[k, 0]`` after ``t`` iterations, is ``>= targets[k]``.  ``tol`` None: no step test; ``targets`` None: no bound
        test, else a scalar or one cut-off per instance, ``+inf`` for an instance without one (a NaN or ``-inf`` is a
        ``ValueError``).  A NaN in either quantity never stops, nor does an instance whose status carries the NaN bit.  A stopped
        instance keeps its multipliers, the x of the top of iteration ``t``, its tie-draw count and its flags and takes no part in
        later launches; ``frozen()`` stays False for it.  ``set_stop(None)`` turns the test off, the state after the constructor.
        No call clears a stopped mark: the tie draws behind a stopped instance are dropped, so it cannot be resumed; a new
        rule applies to the instances still moving, and with the test off the stopped ones stay stopped."""
        if tol is None and targets is None:
            check_every = 1
        else:
            tol, targets, check_every = _check_batch_stop(tol, targets, check_every, self.batch)
        _lib.check(self._l.slp_batch_dga_set_stop(self._h, -1.0 if tol is None else tol, _lib.ptr(targets), check_every))

    def stop_state(self):
        """``(iterations, stopped, step, bound, reason)`` per instance -- int64, bool, float64, float64 and int32 arrays: the
        iterations completed (for a stopped instance its stopping iteration, 0 for a frozen one), whether it is stopped, the last
        evaluated step (``+inf`` before the first check) and bound (``-inf`` before the first check with cut-offs: always a valid
        lower bound) and why it stopped, a bit mask: 0 = moving or frozen, 1 = step, 2 = bound, 3 = both at the same check."""
        iterations, reason = np.zeros(self.batch, dtype=np.int64), np.zeros(self.batch, dtype=np.int32)
        step, bound = np.zeros(self.batch), np.zeros(self.batch)
        _lib.check(self._l.slp_batch_dga_stop_state(self._h, _lib.ptr(iterations), _lib.ptr(reason), _lib.ptr(step), _lib.ptr(bound)))
        return iterations, reason != 0, step, bound, reason


def _check_batch_stop(tol, targets, check_every, batch):
    """The rule of the batch's stopping test, checked without the library: ``(tol, targets, check_every)`` with ``tol`` a float
    or None (no step test), ``targets`` a float64 array of shape ``(batch,)`` or None (no bound test); at least one is given."""
    if tol is None and targets is None:
        raise ValueError("a stopping test needs tol, targets or both: both are None")
    checked, check_every = _many.check_stop(0.0 if tol is None else tol, check_every)
    return (None if tol is None else checked), check_targets(targets, batch), check_every


def dual_gradient_ascent_batch(lp, costs, nb_max_iter=1000, callback_func=None, y_eq=None, y_ineq=None, max_time=None, lower_bounds=None,
                               upper_bounds=None, path=None):
    """``dual_gradient_ascent`` for every row of ``costs`` (shape ``(B, n)``) in place of ``lp.costsvector``, all B solves advancing
    together on the device (an extension: the reference solves one LP per call); returns ``(X, Y_eq, Y_ineq)`` with a leading
    axis B (``Y_ineq`` is None without inequality rows).

    ``lower_bounds`` / ``upper_bounds`` default to the LP's; each of shape ``(n,)`` or ``(B, n)``.  ``y_eq`` / ``y_ineq``: shape
    ``(m,)`` or ``(B, m)``; the default is the reference's seed-0 start, the same for every instance, and every instance's tie
    draws continue that stream from its own position -- so instance k is bit for bit ``dual_gradient_ascent`` on a copy of the LP
    with ``costs[k]`` (and its bounds and start).  An instance whose start is dual infeasible (energy ``-inf``) stands still at
    its start, which is what its single solve returns; the others go on.  ``callback_func(niter, X, 0, 0, elapsed, 0, 0)`` is
    called for ``niter % 100 == 0``; ``max_time`` is tested there and stops the whole batch.  A finite ``b_lower``, a 2-D
    right-hand side (right-hand sides per instance are what ``dual_gradient_ascent_batch_rhs`` takes), a wrong shape, B < 1 or an
    LP without rows raises ``ValueError`` before the library is loaded; a status error raises the single solver's exception,
    naming the instances."""
    return _dga_batch_run(lp, costs, nb_max_iter, callback_func, y_eq, y_ineq, max_time, lower_bounds, upper_bounds, path)[:3]


def dual_gradient_ascent_batch_until(lp, costs, tol=None, targets=None, check_every=10, nb_max_iter=1000, callback_func=None, y_eq=None,
                                     y_ineq=None, max_time=None, lower_bounds=None, upper_bounds=None, path=None):
    """``dual_gradient_ascent_batch`` with a stopping test per instance (extension; the reference runs a fixed number of
    iterations): the batch runs until every instance has stopped or is frozen, at most ``nb_max_iter`` iterations.  Returns
    ``(X, Y_eq, Y_ineq, info)``.

    The test is made on the device (``DeviceDGABatch.set_stop``), at the end of every iteration ``t`` with ``t % check_every == 0``,
    iterations counted from 1: an instance stops iff ``step_t = max|y_t - y_{t-1}| <= tol`` over all its multipliers (the
    inequality part after its clamp; a kind of rows that does not move contributes 0) or its certified lower bound, the dual
    energy of ``y_t``, has reached its cut-off, ``bound_t >= targets[k]``; a NaN never stops.  At least one of ``tol`` (a finite
    float ``>= 0``) and ``targets`` (a scalar or shape ``(B,)``; ``+inf``: no cut-off for that instance; no NaN, no ``-inf``) is
    required, ``check_every`` is an int ``>= 1``: a ``ValueError`` before the library is loaded otherwise, like every shape
    error.  A stopped instance keeps its multipliers and the x of the top of iteration ``t``, bit for bit what
    ``dual_gradient_ascent`` returns for its data with ``nb_max_iter=t``, takes no part in later launches and costs nothing
    more, while the others go on, their iterates unchanged.

    ``info`` is a dict of arrays over the batch: ``iterations`` (int64: completed, for a stopped instance its stopping iteration,
    0 for a frozen one), ``stopped`` (bool; a frozen instance is not stopped), ``reason`` (int32 bit mask: 0 moving or frozen,
    1 step, 2 bound, 3 both at the same check), ``step`` (float64: the last evaluated step, ``+inf`` before the first check) and
    ``lower_bound`` (float64: the dual energy of the returned multipliers, column 0 of the final report -- a certified lower
    bound on the instance's LP value; NaN until the run has ended).

    The cadence of callbacks and of the test of ``max_time`` is that of ``dual_gradient_ascent_batch``.  ``info`` is current at
    every callback: the same dict, updated in place, is set as the ATTRIBUTE ``callback_func.info`` before every call (a function
    or any object that takes attributes; a bound method takes none)."""
    stop = _check_batch_stop(tol, targets, check_every, check_costs(costs, np.size(lp.costsvector))[1])
    return _dga_batch_run(lp, costs, nb_max_iter, callback_func, y_eq, y_ineq, max_time, lower_bounds, upper_bounds, path, stop=stop)


def _check_batch_rhs(lp, batch, b_equalities, b_upper):
    """The right-hand sides of ``dual_gradient_ascent_batch_rhs`` over the rows of ``[A_eq; A_ineq]``, checked without the library:
    shape ``(m,)`` when both kinds are shared, else ``(batch, m)``.  Each kind defaults to the LP's own."""
    parts, batched = [], False
    for name, given, own, a in (("b_equalities", b_equalities, lp.b_equalities, lp.a_equalities), ("b_upper", b_upper, lp.b_upper, lp.a_inequalities)):
        rows = 0 if a is None else a.shape[0]
        if rows:
            v, v_b = check_rhs(name, own if given is None else given, batch, rows, finite=True)
            parts.append(v)
            batched = batched or v_b
    if not batched:
        return np.concatenate(parts) if parts else np.zeros(0)
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(v, (batch, v.shape[-1])) for v in parts], axis=1))


def dual_gradient_ascent_batch_rhs(lp, costs, b_equalities=None, b_upper=None, tol=None, targets=None, check_every=10, nb_max_iter=1000,
                                   callback_func=None, y_eq=None, y_ineq=None, max_time=None, lower_bounds=None, upper_bounds=None, path=None):
    """``dual_gradient_ascent_batch`` / ``dual_gradient_ascent_batch_until`` with right-hand sides per instance (extension): a sweep
    over capacities, budgets or demands, or branch-and-bound nodes that tighten a row.  ``b_equalities`` has shape ``(m_eq,)`` or
    ``(B, m_eq)``, ``b_upper`` ``(m_ineq,)`` or ``(B, m_ineq)``; each defaults to the LP's own 1-D one.  Returns
    ``(X, Y_eq, Y_ineq, info)``.

    Instance k is bit for bit ``dual_gradient_ascent`` on a copy of the LP with ``costs[k]`` and row k of the right-hand sides (and
    its bounds and start): x, y and the tie draws taken.  With ``tol`` and ``targets`` both None the batch runs the fixed horizon
    ``nb_max_iter``; ``info`` -- the dict of ``dual_gradient_ascent_batch_until`` -- then has ``lower_bound`` (the dual energy of the
    returned multipliers against the instance's own right-hand sides, a certified lower bound on its LP value) and ``iterations``
    filled, and nothing stopped.  Otherwise the stopping test, its arguments and ``info`` are those of
    ``dual_gradient_ascent_batch_until``, the bound of instance k being evaluated with its own right-hand sides.

    A finite ``b_lower`` on the LP, a wrong shape, a NaN, or an infinite entry of a batched right-hand side (the message names the
    instance) raises ``ValueError`` before the library is loaded, as do the errors of ``tol``, ``targets`` and ``check_every``."""
    stop, rhs = _check_dga_batch_rhs_call(lp, costs, b_equalities, b_upper, tol, targets, check_every)
    return _dga_batch_rhs_run(lp, costs, rhs, stop, nb_max_iter, callback_func, y_eq, y_ineq, max_time, lower_bounds, upper_bounds, path)


def _check_dga_batch_rhs_call(lp, costs, b_equalities, b_upper, tol, targets, check_every):
    """What ``dual_gradient_ascent_batch_rhs`` checks of its own, without the library: ``(stop, rhs)``, ``stop`` the checked
    ``(tol, targets, check_every)`` or None for the fixed horizon, ``rhs`` as ``_check_batch_rhs`` returns it."""
    batch = check_costs(costs, np.size(lp.costsvector))[1]
    stop = None if tol is None and targets is None else _check_batch_stop(tol, targets, check_every, batch)
    require_one_sided(getattr(lp, "b_lower", None))
    return stop, _check_batch_rhs(lp, batch, b_equalities, b_upper)


def _dga_batch_rhs_run(lp, costs, rhs, stop, nb_max_iter, callback_func, y_eq, y_ineq, max_time, lower_bounds, upper_bounds, path):
    """``dual_gradient_ascent_batch_rhs`` behind its checks (``_check_dga_batch_rhs_call`` gives ``stop`` and ``rhs``)."""
    batch = np.shape(costs)[0]
    out = _dga_batch_run(lp, costs, nb_max_iter, callback_func, y_eq, y_ineq, max_time, lower_bounds, upper_bounds, path, stop=stop, rhs=rhs)
    if stop is not None:
        return out
    x, ye, yi, report, iterations = out
    info = _many.new_stop_info(batch, np.arange(batch))
    info["reason"] = np.zeros(batch, dtype=np.int32)
    info["iterations"][:] = iterations
    info["lower_bound"] = report[:, 0].copy()
    return x, ye, yi, info


def _dga_batch_run(lp, costs, nb_max_iter, callback_func, y_eq, y_ineq, max_time, lower_bounds, upper_bounds, path, stop=None, rhs=None):
    """``dual_gradient_ascent_batch`` plus, as a fourth value, the final ``DeviceDGABatch.report()``; with ``stop`` (the checked
    ``(tol, targets, check_every)`` of ``dual_gradient_ascent_batch_until``) what that function returns.  ``rhs``: the checked
    right-hand sides of ``dual_gradient_ascent_batch_rhs`` in place of the LP's, shape ``(m,)`` or ``(B, m)``; without a stopping
    test the iterations completed per instance are then a fifth value."""
    require_one_sided(getattr(lp, "b_lower", None))
    from .device import DeviceMatrix
    from .tools import CsrArrays

    start = time.perf_counter()
    n = np.size(lp.costsvector)
    costs, batch = check_costs(costs, n)
    a_eq, a_ineq = CsrArrays.from_any(lp.a_equalities), CsrArrays.from_any(lp.a_inequalities)
    m_eq = 0 if a_eq is None else a_eq.shape[0]
    m_in = 0 if a_ineq is None else a_ineq.shape[0]
    if m_eq + m_in == 0:
        raise ValueError("dual_gradient_ascent_batch: the LP has no constraint rows")
    for name, own, rows in (("b_equalities", lp.b_equalities, m_eq), ("b_upper", lp.b_upper, m_in)):
        if rhs is None and rows and np.shape(own) != (rows,):
            raise ValueError(f"{name} has shape {np.shape(own)}: expected ({rows},); per-instance right-hand sides are not built")
    lb, _ = shared_or_batched("lower_bounds", lp.lower_bounds if lower_bounds is None else lower_bounds, batch, n)
    ub, _ = shared_or_batched("upper_bounds", lp.upper_bounds if upper_bounds is None else upper_bounds, batch, n)
    rs = np.random.RandomState(0)   # the reference draws the starts it is not given; the tie draws continue that stream
    ye, ye_b = shared_or_batched("y_eq", -rs.rand(m_eq) if y_eq is None else y_eq, batch, m_eq)
    if y_ineq is None:
        y_ineq = np.abs(rs.rand(m_in)) if a_ineq is not None else np.zeros(0)
    yi, yi_b = shared_or_batched("y_ineq", y_ineq, batch, m_in)
    if ye_b or yi_b:
        y0 = np.concatenate((np.broadcast_to(ye, (batch, m_eq)), np.broadcast_to(yi, (batch, m_in))), axis=1)
    else:
        y0 = np.concatenate((ye, yi))
    if rhs is None:
        b = np.concatenate((_lib.f64(lp.b_equalities) if m_eq else np.zeros(0), _lib.f64(lp.b_upper) if m_in else np.zeros(0)))
    else:
        b = _lib.f64(rhs[0] if rhs.ndim == 2 else rhs)   # the state is created with one vector; the rows follow through set_rhs
    mat = DeviceMatrix.from_blocks(a_eq if m_eq else None, a_ineq if m_in else None, n)
    state = None

    def result():
        ye, yi = state.y()
        return state.x(), ye, (yi if a_ineq is not None else None), state.report()

    try:
        state = DeviceDGABatch(mat, b, costs, lb, ub, y0, m_eq=m_eq, draws=rs.random_sample, path=path)
        if rhs is not None and rhs.ndim == 2:
            state.set_rhs(rhs)
        frozen = state.frozen()
        if stop is None:
            _dga_drive(state, nb_max_iter, callback_func, max_time, start, all_frozen=frozen.all())
            return result() if rhs is None else result() + (state.stop_state()[0],)
        info = _many.new_stop_info(batch, np.arange(batch))
        info["reason"] = np.zeros(batch, dtype=np.int32)
        info["lower_bound"] = np.full(batch, np.nan)
        state.set_stop(*stop)

        def refresh():
            info["iterations"][:], info["stopped"][:], info["step"][:], _, info["reason"][:] = state.stop_state()

        def all_still():
            refresh()
            if callback_func is not None:
                try:
                    callback_func.info = info
                except AttributeError:   # a bound method takes no attribute: wrap it in a function to read ``info``
                    pass
            return bool(np.all(info["stopped"] | frozen))

        _dga_drive(state, nb_max_iter, callback_func, max_time, start, all_frozen=frozen.all(), all_still=all_still)
        x, ye, yi, report = result()
        refresh()
        info["lower_bound"][:] = report[:, 0]
        return x, ye, yi, info
    finally:
        if state is not None:
            state.close()
        mat.close()


# ---- a list of LPs with matrices of their own: one workgroup per LP ------------------------------------------------------------

def _dga_many_lp(k, lp):
    """LP ``k`` of a list, validated (``ValueError``) and brought to the solver's form without touching the library:
    ``(c, lb, ub, eq, b_eq, ineq, b_upper)`` with ``eq`` / ``ineq`` ``CsrArrays`` or None (a block without rows is None)."""
    from .tools import CsrArrays

    try:
        b_lower = getattr(lp, "b_lower", None)
        c = _lib.f64(lp.costsvector)
        a_eq, a_ineq = CsrArrays.from_any(lp.a_equalities), CsrArrays.from_any(lp.a_inequalities)
        lb, ub = _lib.f64(lp.lower_bounds), _lib.f64(lp.upper_bounds)
    except AttributeError as e:
        raise ValueError(f"LP {k} is not an LP object (costsvector, a_equalities, b_equalities, a_inequalities, b_upper, b_lower, "
                         f"lower_bounds, upper_bounds): {e}") from None
    require_one_sided(b_lower, prefix=f"LP {k}: ")
    n = _many.check_cost(k, "costsvector", c).size
    if n > FUSED_MAX:
        raise ValueError(f"LP {k} has {n} variables: the list form holds at most {FUSED_MAX} per LP (one workgroup, breakpoints in "
                         "LDS); an LP with more belongs to the single solver, dual_gradient_ascent")
    for name, v in (("lower_bounds", lb), ("upper_bounds", ub)):
        _many.check_vector(k, name, v, (n,), f"costsvector has {n} entries")
    out = []
    for name, a, rhs_name in (("a_equalities", a_eq, "b_equalities"), ("a_inequalities", a_ineq, "b_upper")):
        if a is None or a.shape[0] == 0:
            out += [None, np.zeros(0)]
            continue
        _many.check_csr(k, name, a, n, f"costsvector has {n} entries")
        out += [a, _many.check_vector(k, rhs_name, getattr(lp, rhs_name), (a.shape[0],), f"{name} has {a.shape[0]} rows")]
    if out[0] is None and out[2] is None:
        raise ValueError(f"LP {k} has no constraint rows")
    return (c, lb, ub) + tuple(out)


def dga_many_start(lps, y_eq=None, y_ineq=None):
    """``(y0s, draw_offsets)`` of the validated LPs: per LP ``[y_eq; y_ineq]`` -- the caller's, or the reference's seed-0 start for
    the LP's own shape (``-rand(m_eq)``, then ``|rand(m_ineq)|``) -- and the position in the seed-0 stream at which the LP's tie
    draws begin: the number of draws its default start took (0 when both parts are given)."""
    count = len(lps)
    given = []
    for name, v in (("y_eq", y_eq), ("y_ineq", y_ineq)):
        if v is None:
            v = [None] * count
        try:
            v = list(v)
        except TypeError:
            v = None
        if v is None or len(v) != count:
            raise ValueError(f"{name} must be None or a sequence of {count} entries, one array (or None) per LP")
        given.append(v)
    y0s, offsets = [], []
    for k, lp in enumerate(lps):
        m_eq = 0 if lp[3] is None else lp[3].shape[0]
        m_in = 0 if lp[5] is None else lp[5].shape[0]
        rs = np.random.RandomState(0)
        parts, taken = [], 0
        for name, v, rows, sign in (("y_eq", given[0][k], m_eq, -1.0), ("y_ineq", given[1][k], m_in, 1.0)):
            if v is None:
                v = -rs.rand(rows) if sign < 0 else np.abs(rs.rand(rows))
                taken += rows
            else:
                v = _many.check_vector(k, name, v, (rows,), f"the LP has {rows} such rows").copy()
            parts.append(v)
        y0s.append(np.concatenate(parts))
        offsets.append(taken)
    return y0s, offsets


def dga_many_system(lps, y0s, draw_offsets):
    """The validated LPs as the arrays ``slp_many_dga_create`` takes -- a dict of:

    ``n``, ``m_eq``, ``m_ineq``, ``draw_offset``: int64 arrays of length ``count``; ``col0``, ``row0``: first column and first row of
    every LP; ``indptr``, ``indices``, ``data``: the CSR rows of all ``K_k = [A_eq,k; A_ineq,k]``, one LP after another, ``indptr``
    running over the whole list, ``indices`` local to the LP and every row in its own storage order; ``b``, ``y0`` in that row order;
    ``c``, ``lb``, ``ub`` concatenated LP by LP.  Needs no GPU."""
    count = len(lps)
    if count < 1:
        raise ValueError("an empty list of LPs")
    n = np.array([lp[0].size for lp in lps], dtype=np.int64)
    m_eq = np.array([0 if lp[3] is None else lp[3].shape[0] for lp in lps], dtype=np.int64)
    m_ineq = np.array([0 if lp[5] is None else lp[5].shape[0] for lp in lps], dtype=np.int64)
    blocks = [(a, rhs) for lp in lps for a, rhs in ((lp[3], lp[4]), (lp[5], lp[6])) if a is not None]
    if int(n.sum()) >= 2 ** 31 or int(m_eq.sum() + m_ineq.sum()) >= 2 ** 31 or sum(a.nnz for a, _ in blocks) >= 2 ** 31:
        raise ValueError("the list has 2^31 or more variables, rows or entries")
    indptr, indices, data = _many.stack_blocks([(a.indptr, a.indices, a.data) for a, _ in blocks])
    y0 = concat(list(y0s), np.float64)
    assert y0.size == int(m_eq.sum() + m_ineq.sum()) and len(draw_offsets) == count
    return dict(n=n, m_eq=m_eq, m_ineq=m_ineq, col0=first_offsets(n), row0=first_offsets(m_eq + m_ineq), indptr=indptr,
                indices=indices, data=data, b=concat([rhs for _, rhs in blocks], np.float64),
                c=concat([lp[0] for lp in lps], np.float64), lb=concat([lp[1] for lp in lps], np.float64),
                ub=concat([lp[2] for lp in lps], np.float64), y0=y0, draw_offset=np.ascontiguousarray(draw_offsets, dtype=np.int64))


class DeviceDGAMany(_DeviceDGA):
    """``DeviceDGA`` for a list of LPs with matrices of their own (``slp_many_dga_*``): one workgroup per LP runs whole iterations
    inside a launch.  ``lps``: the LPs as ``_dga_many_lp`` returns them (each at most ``FUSED_MAX`` variables and at least one
    row); ``y0s``: per LP ``[y_eq; y_ineq]``; ``draw_offsets``: per LP the position in the stream of draws at which its tie draws
    begin (``dga_many_start`` gives both).  ``draws(count)`` gives the next ``count`` draws of that one stream FROM ITS START
    (default: a private ``RandomState(0)``); every LP reads it at its own position.  Results are lists of per-LP arrays.  An LP
    whose start has dual energy ``-inf`` is frozen (``frozen()``): its x and y stay the start's."""

    _PREFIX = "many_dga"
    _WHERE = "LPs {} of the list"

    def __init__(self, lps, y0s, draw_offsets, draws=None):
        s = dga_many_system(lps, y0s, draw_offsets)
        self.count = len(lps)
        self.n, self.m_eq, self.m = s["n"], s["m_eq"], s["m_eq"] + s["m_ineq"]
        self.system = s
        self._draws = draws if draws is not None else np.random.RandomState(0).random_sample
        # all of the above needs no GPU; the library is loaded (and bound to a device) only now
        self._l = _lib.lib()
        self._h = _lib.check_handle(self._l.slp_many_dga_create(
            self.count, _lib.ptr(s["n"]), _lib.ptr(s["m_eq"]), _lib.ptr(s["m_ineq"]), _lib.ptr(s["indptr"]), _lib.ptr(s["indices"]),
            _lib.ptr(s["data"]), _lib.ptr(s["b"]), _lib.ptr(s["c"]), _lib.ptr(s["lb"]), _lib.ptr(s["ub"]), _lib.ptr(s["y0"]),
            _lib.ptr(s["draw_offset"])))

    def kmax(self):
        """Iterations one launch holds at most (from the shapes; ``SLP_DGA_MANY_KMAX`` lowers it)."""
        return int(self._l.slp_many_dga_kmax(self._h))

    def status(self):
        """``(flags[count], tie draws taken[count], draws left in the buffer behind the furthest position, iterations done)``;
        reading it synchronises."""
        out = np.zeros(2 * self.count + 2, dtype=np.int64)
        _lib.check(self._l.slp_many_dga_status(self._h, _lib.ptr(out)))
        per = out[:2 * self.count].reshape(self.count, 2)
        return per[:, 0].copy(), per[:, 1].copy(), int(out[-2]), int(out[-1])

    def frozen(self):
        out = np.zeros(self.count, dtype=np.int32)
        _lib.check(self._l.slp_many_dga_frozen(self._h, _lib.ptr(out)))
        return out.astype(bool)

    def x(self):
        out = np.empty(int(self.n.sum()))
        _lib.check(self._l.slp_many_dga_get_x(self._h, _lib.ptr(out)))
        return split_by(out, self.n)

    def y(self):
        """``(y_eqs, y_ineqs)``: two lists of per-LP arrays."""
        out = np.empty(int(self.m.sum()))
        _lib.check(self._l.slp_many_dga_get_y(self._h, _lib.ptr(out)))
        both = split_by(out, self.m)
        return [v[:me].copy() for v, me in zip(both, self.m_eq)], [v[me:].copy() for v, me in zip(both, self.m_eq)]

    def report(self):
        """Array of shape ``(count, 3)``: per LP ``(dual energy, largest violation, sum of violations)`` of its multipliers as they
        are, x their dual argmin.  Column 0 is a certified lower bound on the LP's value."""
        out = np.zeros((self.count, 3))
        _lib.check(self._l.slp_many_dga_report(self._h, _lib.ptr(out)))
        return out

    def set_stop(self, tol, check_every=1):
        """Arms the per-LP stopping test of the iteration kernel (``slp_many_dual_set_stop``): at the end of every iteration ``t``
        of an LP with ``t % check_every == 0`` -- counted from 1 over the LP's life -- the LP stops iff ``max|y_t - y_{t-1}| <=
        tol`` over all its multipliers (the inequality part after its clamp; a NaN never stops, nor does an LP whose status
        carries the NaN bit); a stopped LP keeps its multipliers, its x, its tie-draw count and its flags and takes no part in
        later calls.  ``tol=None`` turns the test off, the state after the constructor.  Unlike ``CPManyState.set_stop`` no call
        clears a stopped flag: the tie draws behind a stopped LP are dropped, so it cannot be resumed; a new tolerance or
        cadence applies to the LPs still moving, and with the test off the stopped LPs stay stopped."""
        if tol is None:
            tol, check_every = -1.0, 1
        else:
            tol, check_every = _many.check_stop(tol, check_every)
        _lib.check(self._l.slp_many_dual_set_stop(self._h, tol, check_every))

    def stop_state(self):
        """``(iterations, stopped, step)`` per LP, int64, bool and float64 arrays: the iterations completed (for a stopped LP its
        stopping iteration, 0 for a frozen one), whether it is stopped and the last evaluated step (``+inf`` before the first
        test)."""
        iterations, stopped, step = np.zeros(self.count, dtype=np.int64), np.zeros(self.count, dtype=np.int32), np.zeros(self.count)
        _lib.check(self._l.slp_many_dual_stop_state(self._h, _lib.ptr(iterations), _lib.ptr(stopped), _lib.ptr(step)))
        return iterations, stopped.astype(bool), step

    def set_cutoff(self, tol, check_every=1, targets=None):
        """``set_stop`` with a cut-off for each LP's bound as well (``slp_many_dual_set_cutoff``): at the end of every iteration
        ``t`` of an LP with ``t % check_every == 0`` the LP stops iff ``max|y_t - y_{t-1}| <= tol`` or its dual energy, bit for bit
        ``report()[k, 0]`` after ``t`` iterations, is ``>= targets[k]``; both are looked at.  ``tol`` None: no step test (the step is
        still recorded); ``targets`` None: no bound test -- ``set_cutoff(tol, check_every)`` is ``set_stop(tol, check_every)`` --
        else a scalar or one cut-off per LP, ``+inf`` for an LP without one (a NaN or ``-inf`` is a ``ValueError``); both None turn
        the test off.  While cut-offs are armed the bound of every moving LP is evaluated and recorded at every check, inside the
        iteration kernel.  A NaN in either quantity never stops, nor does an LP whose status carries the NaN bit.  With cut-offs
        an LP of more than 65536 rows is refused (``SlpError``).  As with ``set_stop`` a stopped LP keeps its multipliers, the x
        of the top of iteration ``t``, its tie-draw count and its flags, takes no part in later launches and cannot be resumed;
        a new rule applies to the LPs still moving."""
        if tol is None and targets is None:
            check_every = 1
        else:
            tol, targets, check_every = _check_batch_stop(tol, targets, check_every, self.count)
        _lib.check(self._l.slp_many_dual_set_cutoff(self._h, -1.0 if tol is None else tol, _lib.ptr(targets), check_every))

    def stop_state_full(self):
        """``(iterations, stopped, step, bound, reason)`` per LP -- int64, bool, float64, float64 and int32 arrays, as
        ``DeviceDGABatch.stop_state``: the first three are ``stop_state()``, ``bound`` is the last evaluated bound (``-inf`` before
        the first check with cut-offs: always a valid lower bound) and ``reason`` why the LP stopped, a bit mask: 0 = moving or
        frozen, 1 = step, 2 = bound, 3 = both at the same check."""
        iterations, reason = np.zeros(self.count, dtype=np.int64), np.zeros(self.count, dtype=np.int32)
        step, bound = np.zeros(self.count), np.zeros(self.count)
        _lib.check(self._l.slp_many_dual_cutoff_state(self._h, _lib.ptr(iterations), _lib.ptr(reason), _lib.ptr(step), _lib.ptr(bound)))
        return iterations, reason != 0, step, bound, reason

    def set_compaction(self, on=True):
        """Turns compaction on or off (``slp_many_dual_set_compaction``; off after the constructor).  While it is on, every
        iteration launch of a call on a state that is armed, or has a stopped or a frozen LP, runs over a list of the live LPs --
        neither frozen nor stopped -- that the device builds in front of it: the live LPs get consecutive workgroups, the grid is
        the number of LPs live when the call began, and the iterations one launch holds are those of that many workgroups.  Every
        LP's x, y, tie draws, flags, stop record and report are bit for bit those of the state without it."""
        if not isinstance(on, (bool, int, np.integer)) or int(on) not in (0, 1):
            raise ValueError(f"on must be True or False, not {on!r}")
        _lib.check(self._l.slp_many_dual_set_compaction(self._h, int(on)))

    def live_state(self):
        """``(live, order, launched, cap)`` (``slp_many_dual_live_state``): the number of live LPs, their numbers in the order of the
        device's list (an int32 array of length ``live``, increasing), the number of workgroups of the last iteration launch and the
        iterations per launch the last ``iterate`` call that launched anything was held to (both 0 before the first).  Works with
        compaction on or off; reading it synchronises."""
        live, launched, cap = (np.zeros(1, dtype=np.int64) for _ in range(3))
        order = np.zeros(self.count, dtype=np.int32)
        _lib.check(self._l.slp_many_dual_live_state(self._h, _lib.ptr(live), _lib.ptr(order), _lib.ptr(launched), _lib.ptr(cap)))
        assert np.all(order[int(live[0]):] == -1)
        return int(live[0]), order[:int(live[0])].copy(), int(launched[0]), int(cap[0])


def dual_gradient_ascent_many(lps, nb_max_iter=1000, callback_func=None, y_eq=None, y_ineq=None, max_time=None):
    """``dual_gradient_ascent`` on every LP of ``lps`` -- LPs whose constraint matrices differ -- all advancing together on the
    device, one workgroup per LP (an extension: the reference solves one LP per call); returns ``(xs, y_eqs, y_ineqs)``, lists of
    per-LP arrays (``y_ineqs[k]`` is None where ``lps[k].a_inequalities`` is None).

    ``lps``: a sequence of objects with the reference's attributes, as ``dual_gradient_ascent`` takes; every LP has at most
    ``FUSED_MAX`` = 8192 variables (an LP with more belongs to ``dual_gradient_ascent``).  ``y_eq`` / ``y_ineq``: None, or one
    entry (or None) per LP.  The default start of LP k is the reference's seed-0 start for its own shape and its tie draws
    continue that stream, so LP k is bit for bit ``dual_gradient_ascent`` on ``lps[k]``.  An LP whose start is dual infeasible
    (energy ``-inf``) stands still at its start, which is what its single solve returns; the others go on.
    ``callback_func(niter, xs, 0, 0, elapsed, 0, 0)`` is called for ``niter % 100 == 0``; ``max_time`` is tested there and stops
    the whole list.  A finite ``b_lower``, a shape error, an LP without rows or with more than 8192 variables, or an empty list
    raises ``ValueError`` naming the LP, before the library is loaded; a status error raises the single solver's exception,
    naming the LPs."""
    return _dga_many_run(lps, nb_max_iter, callback_func, y_eq, y_ineq, max_time)[:3]


def dual_gradient_ascent_many_until(lps, tol, check_every=10, nb_max_iter=1000, callback_func=None, y_eq=None, y_ineq=None, max_time=None):
    """``dual_gradient_ascent_many`` with a stopping test per LP (extension; the reference runs a fixed number of iterations): the
    list runs until every LP has stopped or is frozen, at most ``nb_max_iter`` iterations.  Returns ``(xs, y_eqs, y_ineqs, info)``.

    The test is made inside the iteration kernel (``DeviceDGAMany.set_stop``), at the end of every iteration ``t`` of an LP with
    ``t % check_every == 0``, iterations counted from 1: the LP stops iff ``step_t = max|y_t - y_{t-1}| <= tol`` over all its
    multipliers ``y_t = [y_eq; y_ineq]`` after ``t`` iterations (the inequality part after its clamp; a kind of rows that does not
    move contributes 0; a NaN never stops).  A stopped LP keeps its multipliers and the x of the top of iteration ``t``, bit for bit
    what ``dual_gradient_ascent(None, lps[k], nb_max_iter=t)`` returns, while the others go on.  ``tol`` is a finite float ``>= 0``,
    ``check_every`` an int ``>= 1``: a ``ValueError`` before the library is loaded otherwise, like every shape error.

    ``info`` is a dict of arrays over the list: ``iterations`` (int64: completed, for a stopped LP its stopping iteration, 0 for a
    frozen one), ``stopped`` (bool; a frozen LP is not stopped), ``step`` (float64: the last evaluated step, ``+inf`` before the
    first test) and ``lower_bound`` (float64: the dual energy of the returned multipliers, column 0 of the final report -- a
    certified lower bound on the LP's value; NaN until the run has ended).

    The cadence of callbacks and of the test of ``max_time`` is that of ``dual_gradient_ascent_many``: ``callback_func(niter, xs,
    0, 0, elapsed, 0, 0)`` for ``niter % 100 == 0``, where ``xs[k]`` of an LP stopped at or before ``niter`` is its final x.
    ``info`` is current at every callback: the same dict, updated in place, is set as the ATTRIBUTE ``callback_func.info`` before
    every call (a function or any object that takes attributes; a bound method takes none)."""
    stop = _many.check_stop(tol, check_every)
    xs, y_eqs, y_ineqs, report, info = _dga_many_run(lps, nb_max_iter, callback_func, y_eq, y_ineq, max_time, stop=stop)
    return xs, y_eqs, y_ineqs, info


def dual_gradient_ascent_many_cutoff(lps, tol, check_every=10, nb_max_iter=1000, callback_func=None, y_eq=None, y_ineq=None, max_time=None,
                                     targets=None):
    """``dual_gradient_ascent_many_until`` with a cut-off for each LP's certified lower bound as well -- nodes of a branch and bound,
    whose matrices differ: an LP whose bound has passed the incumbent is pruned and costs nothing more.  Returns ``(xs, y_eqs,
    y_ineqs, info)``.

    At the end of every iteration ``t`` of an LP with ``t % check_every == 0``, inside the iteration kernel
    (``DeviceDGAMany.set_cutoff``), the LP stops iff ``step_t = max|y_t - y_{t-1}| <= tol`` or ``bound_t``, the dual energy of
    ``y_t``, is ``>= targets[k]``; both are looked at, a NaN never stops.  At least one of ``tol`` (a finite float ``>= 0``, or None:
    no step test) and ``targets`` (a scalar or one value per LP; ``+inf``: no cut-off for that LP; no NaN, no ``-inf``; or None: no
    bound test, which is ``dual_gradient_ascent_many_until``) is required, ``check_every`` is an int ``>= 1``: a ``ValueError`` before
    the library is loaded otherwise.  With ``targets`` every LP has at most 65536 rows.

    ``info`` is that of ``dual_gradient_ascent_many_until`` and, with ``targets``, also has ``bound`` (float64: the last bound
    evaluated at a check, ``-inf`` before the first) and ``reason`` (int32 bit mask: 0 moving or frozen, 1 step, 2 bound, 3 both at
    the same check).  For an LP stopped at a check with cut-offs ``info["lower_bound"][k] == info["bound"][k]``, bit for bit."""
    return _dga_many_stopping(lps, tol, check_every, nb_max_iter, callback_func, y_eq, y_ineq, max_time, targets, False)


def dual_gradient_ascent_many_compact(lps, tol, check_every=10, nb_max_iter=1000, callback_func=None, y_eq=None, y_ineq=None, max_time=None,
                                      targets=None):
    """``dual_gradient_ascent_many_cutoff`` with compaction on (``DeviceDGAMany.set_compaction``): the same arguments, the same
    refusals before the library is loaded, and ``(xs, y_eqs, y_ineqs, info)`` bit for bit the same.  The LPs still moving are handed
    consecutive workgroups in every launch, so a list in which LPs are retired here and there -- the pruned nodes of a branch and
    bound -- keeps the whole device busy, launches only as many workgroups as LPs are left and holds more iterations per launch
    as the list thins out."""
    return _dga_many_stopping(lps, tol, check_every, nb_max_iter, callback_func, y_eq, y_ineq, max_time, targets, True)


def _dga_many_stopping(lps, tol, check_every, nb_max_iter, callback_func, y_eq, y_ineq, max_time, targets, compact):
    """``dual_gradient_ascent_many_cutoff`` and ``dual_gradient_ascent_many_compact``: the checks and the run they share (with
    ``targets`` None the test is that of ``dual_gradient_ascent_many_until``)."""
    try:
        lps = list(lps)
    except TypeError:
        raise ValueError("lps must be a sequence of LP objects") from None
    if targets is None and tol is not None:
        stop, cutoff = _many.check_stop(tol, check_every), None
    else:
        stop, cutoff = None, _check_batch_stop(tol, targets, check_every, len(lps))
    xs, y_eqs, y_ineqs, report, info = _dga_many_run(lps, nb_max_iter, callback_func, y_eq, y_ineq, max_time, stop=stop, cutoff=cutoff,
                                                     compact=compact)
    return xs, y_eqs, y_ineqs, info


def _dga_many_run(lps, nb_max_iter, callback_func, y_eq, y_ineq, max_time, frozen_out=None, stop=None, cutoff=None, compact=False):
    """``dual_gradient_ascent_many`` plus, as a fourth value, the final ``DeviceDGAMany.report()`` and, as a fifth, the ``info`` of
    ``dual_gradient_ascent_many_until`` (``stop`` the checked ``(tol, check_every)``) or of ``dual_gradient_ascent_many_cutoff``
    (``cutoff`` the checked ``(tol, targets, check_every)``); None without a stopping test.  ``frozen_out``: a list that receives
    the frozen flags before the first iteration.  ``compact``: the run is made with ``DeviceDGAMany.set_compaction`` on."""
    start = time.perf_counter()
    try:
        lps = list(lps)
    except TypeError:
        raise ValueError("lps must be a sequence of LP objects") from None
    if len(lps) < 1:
        raise ValueError("an empty list of LPs")
    forms = [_dga_many_lp(k, lp) for k, lp in enumerate(lps)]
    y0s, offsets = dga_many_start(forms, y_eq, y_ineq)
    has_ineq = [getattr(lp, "a_inequalities", None) is not None for lp in lps]
    state = DeviceDGAMany(forms, y0s, offsets, draws=np.random.RandomState(0).random_sample)
    try:
        if compact:
            state.set_compaction(True)
        frozen = state.frozen()
        if frozen_out is not None:
            frozen_out[:] = frozen.tolist()
        info, all_still = None, None
        if stop is not None or cutoff is not None:
            everyone = np.arange(state.count)
            info = _many.new_stop_info(state.count, everyone)
            info["lower_bound"] = np.full(state.count, np.nan)
            if cutoff is not None:
                info["bound"] = np.full(state.count, -np.inf)
                info["reason"] = np.zeros(state.count, dtype=np.int32)
                state.set_cutoff(cutoff[0], cutoff[2], cutoff[1])
            else:
                state.set_stop(*stop)

            def refresh():
                if cutoff is None:
                    _many.spread_stop_state(info, everyone, state.stop_state())
                else:
                    info["iterations"][:], info["stopped"][:], info["step"][:], info["bound"][:], info["reason"][:] = state.stop_state_full()

            def all_still():
                refresh()
                if callback_func is not None:
                    try:
                        callback_func.info = info
                    except AttributeError:   # a bound method takes no attribute: wrap it in a function to read ``info``
                        pass
                return bool(np.all(info["stopped"] | frozen))

        _dga_drive(state, nb_max_iter, callback_func, max_time, start, all_frozen=frozen.all(), all_still=all_still)
        yes, yis = state.y()
        report = state.report()
        if info is not None:
            refresh()
            info["lower_bound"][:] = report[:, 0]
        return state.x(), yes, [yi if h else None for yi, h in zip(yis, has_ineq)], report, info
    finally:
        state.close()
