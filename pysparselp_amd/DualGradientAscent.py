"""Gradient ascent in the dual with an exact line search, on the GPU (reference DualGradientAscent.py:36-245).

The dual function of ``min c.x, A_e x = b_e, A_i x <= b_u, lb <= x <= ub`` is concave and piecewise linear in the multipliers;
every iteration moves the inequality multipliers, then the equality multipliers, along their (masked) gradient to the exact
maximiser on that line -- a sort of the breakpoints ``-c_bar_j / d_j``, two running sums and a bisection
(csrc/slp_dga.hip).  The multipliers it returns are dual feasible, so their dual energy (``DeviceDGA.report``) is a certified
lower bound on the LP's value.
"""
import os
import time

import numpy as np

from . import _lib

PATHS = {"auto": 0, "fused": 1, "general": 2}
FUSED_MAX = 8192    # most variables of the fused search (one workgroup, breakpoints in LDS)
FUSED_AUTO = 2048   # ... and up to where it is the default (beyond, the general search is faster)
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


class DeviceDGA:
    """The iteration state on the device (``slp_dga_*``): ``a`` a ``DeviceMatrix`` (any product format, chunked included) whose
    first ``m_eq`` rows are the equalities, ``b`` = ``[b_eq; b_upper]``, ``y0`` the start multipliers, ``draws`` a callable
    ``draws(count)`` giving the next ``count`` uniform draws of the tie rule (default: a private ``RandomState(0)``).
    ``path``: ``"auto"`` (the fused one-workgroup search up to ``FUSED_AUTO`` variables, else the general one), ``"fused"``
    (at most ``FUSED_MAX`` variables), ``"general"``; the environment's ``SLP_DGA_PATH`` picks it when ``path`` is None."""

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

    def close(self):
        if getattr(self, "_h", None):
            self._l.slp_dga_destroy(self._h)
            self._h = None

    __del__ = close

    def path(self):
        return {1: "fused", 2: "general"}[int(self._l.slp_dga_path(self._h))]

    def status(self):
        """``(flags, tie draws taken, draws left in the buffer, iterations done)``; reading it synchronises."""
        out = np.zeros(4, dtype=np.int64)
        _lib.check(self._l.slp_dga_status(self._h, _lib.ptr(out)))
        return tuple(int(v) for v in out)

    def push_random(self, values):
        values = _lib.f64(values)
        _lib.check(self._l.slp_dga_push_random(self._h, _lib.ptr(values), values.size))

    def iterate(self, k, refill=True):
        """``k`` iterations, nothing read back in between.  ``refill``: the draw buffer is topped up to two draws per iteration
        first; without it the call stops early when the buffer could run dry (``status()[3]`` tells how far it got)."""
        k = int(k)
        if refill:
            left = self.status()[2]
            if left < 2 * k:
                self.push_random(self._draws(2 * k - left))
        _lib.check(self._l.slp_dga_iterate(self._h, k))

    def check(self):
        flags = self.status()[0]
        _check_status(flags & ~STATUS_DRAWS_DRY)
        return flags

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

    def timing(self, on):
        _lib.check(self._l.slp_dga_timing(self._h, int(bool(on))))

    def timing_read(self):
        """Milliseconds per stage since ``timing(True)``: products, sort, scans, rest, fused search."""
        out = np.zeros(5)
        _lib.check(self._l.slp_dga_timing_read(self._h, _lib.ptr(out)))
        return dict(zip(("products", "sort", "scans", "rest", "fused_search"), (float(v) for v in out)))


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
    b_lower = getattr(lp, "b_lower", None)
    if b_lower is not None and np.size(b_lower) > 0 and np.max(b_lower) != -np.inf:
        raise ValueError("dual_gradient_ascent needs one-sided inequalities: b_lower must be None or all -inf")
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
        i = 0
        while i < nb_max_iter:
            k = 1 if i % 100 == 0 else min(100 - i % 100, nb_max_iter - i)
            state.iterate(k)
            i += k
            state.check()
            if (i - 1) % 100 == 0:
                elapsed = time.perf_counter() - start
                if callback_func is not None:
                    callback_func(i - 1, state.x(), 0, 0, elapsed, 0, 0)
                if max_time is not None and elapsed > max_time:
                    break
        return result(state.x())
    finally:
        if state is not None:
            state.close()
        mat.close()
