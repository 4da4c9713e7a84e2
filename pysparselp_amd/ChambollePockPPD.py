"""Chambolle-Pock LP solver: host driver over the HIP kernels.

Drop-in for ``pysparselp.ChambollePockPPD.chambolle_pock_ppd``
(reference ChambollePockPPD.py:36-346): same signature, same callback contract
``callback_func(niter, x, energy1, energy2, elapsed, max_violated_equality,
max_violated_inequality)`` every ``nb_iter_plot`` iterations (including
iteration 0), same return value ``(x[:n], best_integer_solution)``.

The host keeps only the control flow; the preconditioners, every SpMV / SpMV^T,
the projections and the report reductions run on the GPU
(pysparselp_amd/csrc/slp_cp.hip) through the C ABI of include/slp_hip.h.

``chambolle_pock_ppd_batch`` (extension) solves B LPs that share the constraint
matrices and differ in ``c`` (optionally in the right-hand sides, the bounds and
``x0``) together: two launches per iteration for all of them
(pysparselp_amd/csrc/slp_cp_batch.hip).
"""
import time

import numpy as np

from . import _lib
from . import _many
from ._cp_gap import CPGapMethods, check_gap, vertex_certificate
from ._batch import box_vertex, concat, first_offsets, shared_or_batched, split_by
from ._lib import ORDER_AUTO
from .parallel import collective_elapsed


def _take_rows(a, rows, sign):
    """CSR rows ``rows`` of ``a`` (entry order kept), values times ``sign``."""
    indptr, indices, data = _lib.csr_arrays(a)
    cnt = (indptr[1:] - indptr[:-1])[rows]
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(cnt, out=ptr[1:])
    src = np.repeat(indptr[rows] - ptr[:-1], cnt) + np.arange(ptr[-1])
    return ptr, indices[src], sign * data[src]


def one_sided_system(a_ineq, b_lower, b_upper):
    """``b_lower <= A x <= b_upper``  ->  ``K x <= b`` (reference :74-88).

    Returns raw CSR arrays ``(indptr, indices, data, nrows)`` and ``b``: rows
    with a finite upper bound first, then the negated rows with a finite lower
    bound; when no lower bound is finite the matrix is returned untouched.
    """
    indptr, indices, data = _lib.csr_arrays(a_ineq)
    if b_lower is None:
        return (indptr, indices, data, a_ineq.shape[0]), _lib.f64(b_upper)
    b_lower, b_upper = _lib.f64(b_lower), _lib.f64(b_upper)
    up = np.nonzero(b_upper != np.inf)[0]
    lo = np.nonzero(b_lower != -np.inf)[0]
    b = np.hstack((b_upper[up], -b_lower[lo]))
    if len(lo) > 0 and len(up) > 0:
        p1, j1, v1 = _take_rows(a_ineq, up, 1.0)
        p2, j2, v2 = _take_rows(a_ineq, lo, -1.0)
        mat = (np.concatenate((p1, p1[-1] + p2[1:])), np.concatenate((j1, j2)), np.concatenate((v1, v2)), len(up) + len(lo))
    elif len(lo) > 0:
        mat = (indptr, indices, -data, a_ineq.shape[0])
    else:
        mat = (indptr, indices, data, a_ineq.shape[0])
    return mat, b


class CPState(CPGapMethods):
    """Device-resident Chambolle-Pock state (thin RAII wrapper of ``slp_cp``); ``certificate``, ``set_stop_gap`` and ``gap_state``
    are ``_cp_gap.CPGapMethods``'."""

    def __init__(self, c, a_eq, beq, ineq, b_ineq, lb, ub, x0, alpha, theta, order=ORDER_AUTO):
        self._l = _lib.lib()
        c, lb, ub = _lib.f64(c), _lib.f64(lb), _lib.f64(ub)
        self.n = c.size
        parts_ptr, parts_idx, parts_val, parts_b = [np.zeros(1, dtype=np.int64)], [], [], []
        self.m_eq = 0
        if a_eq is not None:
            p, j, v = _lib.csr_arrays(a_eq)
            self.m_eq = a_eq.shape[0]
            parts_ptr.append(p[1:])
            parts_idx.append(j)
            parts_val.append(v)
            parts_b.append(_lib.f64(beq))
        self.m_ineq = 0
        if ineq is not None:
            p, j, v, rows = ineq
            self.m_ineq = rows
            off = parts_ptr[-1][-1] if len(parts_ptr) > 1 else 0
            parts_ptr.append(off + p[1:])
            parts_idx.append(j)
            parts_val.append(v)
            parts_b.append(_lib.f64(b_ineq))
        indptr = np.ascontiguousarray(np.concatenate(parts_ptr), dtype=np.int64)
        indices = np.ascontiguousarray(np.concatenate(parts_idx) if parts_idx else np.zeros(0), dtype=np.int32)
        data = _lib.f64(np.concatenate(parts_val) if parts_val else np.zeros(0))
        b = _lib.f64(np.concatenate(parts_b) if parts_b else np.zeros(0))
        if indices.size and (indices.min() < 0 or indices.max() >= self.n):
            raise ValueError("constraint matrix has a column index outside [0, n)")
        # under a communicator (parallel.init_comm_from_env): every rank holds the LP and hands over only its block of the
        # stacked rows K = [A_eq; A_ineq]; x, c, T, lb, ub are replicated, one all-reduce of n doubles per iteration
        from .parallel import local_rows

        r0, r1, m_eq_local = local_rows(indptr, self.m_eq)
        if (r0, r1) != (0, indptr.size - 1):
            k0, k1 = int(indptr[r0]), int(indptr[r1])
            indptr = np.ascontiguousarray(indptr[r0:r1 + 1] - k0)
            indices, data, b = np.ascontiguousarray(indices[k0:k1]), np.ascontiguousarray(data[k0:k1]), np.ascontiguousarray(b[r0:r1])
            self.m_eq, self.m_ineq = m_eq_local, (r1 - r0) - m_eq_local
        x0 = _lib.f64(x0) if x0 is not None else None
        self._h = _lib.check_handle(self._l.slp_cp_create(
            self.n, self.m_eq, self.m_ineq, _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(data), _lib.ptr(b),
            _lib.ptr(c), _lib.ptr(lb), _lib.ptr(ub), _lib.ptr(x0), float(alpha), float(theta), int(order)))

    def close(self):
        if getattr(self, "_h", None):
            self._l.slp_cp_destroy(self._h)
            self._h = None

    __del__ = close

    def iterate(self, k):
        _lib.check(self._l.slp_cp_iterate(self._h, int(k)))

    def primal_step(self):
        _lib.check(self._l.slp_cp_primal_step(self._h))

    def dual_step(self):
        _lib.check(self._l.slp_cp_dual_step(self._h))

    def report(self):
        out = np.zeros(8)
        _lib.check(self._l.slp_cp_report(self._h, _lib.ptr(out)))
        return out

    def x(self):
        out = np.empty(self.n)
        _lib.check(self._l.slp_cp_get_x(self._h, _lib.ptr(out)))
        return out

    def y(self):
        out = np.empty(self.m_eq + self.m_ineq)
        _lib.check(self._l.slp_cp_get_y(self._h, _lib.ptr(out)))
        return out

    def preconditioners(self):
        t, s = np.empty(self.n), np.empty(self.m_eq + self.m_ineq)
        _lib.check(self._l.slp_cp_get_preconditioners(self._h, _lib.ptr(t), _lib.ptr(s)))
        return t, s

    def bench(self, k):
        ms = np.zeros(3)
        _lib.check(self._l.slp_cp_bench(self._h, int(k), _lib.ptr(ms)))
        return ms


def device_cp(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0=None, alpha=1, theta=1, order=ORDER_AUTO, remove_fixed=False):
    """The Chambolle-Pock state of the LP as ``chambolle_pock_ppd`` receives it, set up on the device (``setup="device"``):
    ``[A_eq; A_ineq]`` is stacked on the device (``DeviceMatrix.from_blocks``, or row chunks when it would not fit,
    ``host_setup.upload``) and ``DeviceCP`` does the one-sided stacking (``gather_rows``) and, with ``remove_fixed``, the
    removal of fixed variables of ``SparseLP.solve`` (SparseLP.py:1244-1248).  Under a communicator this rank's rows only.
    Returns ``(state, free, shift)``: ``state.x_reduced()`` is the iterate over the free variables."""
    from . import host_setup
    from .scale import DeviceCP, one_sided_rows

    c, lb, ub = _lib.f64(c), _lib.f64(lb), _lib.f64(ub)
    n = c.size
    (e0, e1), (i0, i1) = host_setup.local_blocks(a_eq, a_ineq)
    eq, ineq = host_setup.rows_of(a_eq, e0, e1), host_setup.rows_of(a_ineq, i0, i1)
    m_eq, m_in = e1 - e0, i1 - i0
    # the stacked right-hand sides: [b_eq; b_upper] and [-inf; b_lower] (None bounds: +inf / -inf)
    part = lambda v, r0, r1, fill, k: np.full(k, fill) if v is None else _lib.f64(v)[r0:r1]  # noqa: E731
    bu = np.concatenate((part(beq, e0, e1, 0.0, m_eq), part(b_upper, i0, i1, np.inf, m_in)))
    bl = None if b_lower is None else np.concatenate((np.full(m_eq, -np.inf), _lib.f64(b_lower)[i0:i1]))
    entries = host_setup.chunk_entries(host_setup.nnz_of(eq, ineq), m_eq + m_in, n)
    free = (ub > lb) if remove_fixed else np.ones(n, dtype=bool)
    shift = np.where(free, 0.0, lb)
    if entries is None:
        mat, _ = host_setup.upload(eq, ineq, n)
        try:
            state = DeviceCP(mat, bu, c, lb, ub, alpha=alpha, theta=theta, order=order, m_eq=m_eq, b_lower=bl, remove_fixed=remove_fixed,
                             x0=x0)
        except BaseException:
            mat.close()
            raise
        if state.a is mat:
            state._owned = mat
        else:
            mat.close()   # the solver works on a derived copy (fixed variables removed, one-sided stacking)
        return state, free, shift
    # chunked: the one-sided stacking needs row gathers, which a chunked matrix (no CSR) cannot serve
    if bl is not None and one_sided_rows(m_eq + m_in, m_eq, bl, bu) is not None:
        raise ValueError("this LP needs a chunked matrix on one GPU, and Chambolle-Pock with lower-bounded inequality rows needs the "
                         f"one-sided stacking (gather_rows), which a chunked matrix cannot serve; {host_setup.MULTI_GPU}")
    keep = None if free.all() else free
    mat, a_shift = host_setup.upload(eq, ineq, n, entries, keep=keep, shift=None if keep is None else shift)
    try:
        if keep is not None:  # the fixed variables went chunk by chunk (remove_fixed_variables, SparseLP.py:632-674)
            bu = bu - a_shift
            c, lb, ub = c[free], lb[free], ub[free]
            x0 = None if x0 is None else _lib.f64(x0)[free]
        state = DeviceCP(mat, bu, c, lb, ub, alpha=alpha, theta=theta, order=order, m_eq=m_eq, x0=x0)
    except BaseException:
        mat.close()
        raise
    state._owned = mat
    return state, free, shift


def _cp_loop(state, c, n, has_ineq, nb_max_iter, nb_iter_plot, callback_func, max_time, start, x_of, stopped_now=None):
    """The reporting loop of chambolle_pock_ppd (:195-343) over a solver state; ``x_of(state)`` is its iterate.
    Returns ``(x, best_integer_solution)``.

    ``stopped_now()`` (a state armed with ``set_stop_gap``; ``None``: no test) is asked before every report's primal half whether
    the state is stopped: the loop ends there, without a report.  A stopped state ignores ``iterate``, so ``niter`` may run ahead
    of the state's own count until then."""
    best_integer_solution_energy = np.inf
    best_integer_solution = None
    niter = 0
    while niter < nb_max_iter:
        if niter % nb_iter_plot == 0:
            if stopped_now is not None and stopped_now():
                break
            state.primal_step()
            elapsed = time.perf_counter() - start
            if (max_time is not None) and collective_elapsed(elapsed) > max_time:  # the same decision on every rank
                break
            energy1, energy2, max_violated_equality, max_violated_inequality, max_eq_at_x = state.report()[:5]
            if not has_ineq:
                max_violated_inequality = 0  # the reference dereferences a_ineq here (:283) and fails
            x = None
            if max_eq_at_x == 0 and max_violated_inequality <= 0:  # :284-291 with force_integer=False
                x = x_of(state)
                energy_rounded = c.dot(x)
                if energy_rounded < best_integer_solution_energy:
                    best_integer_solution_energy = energy_rounded
                    best_integer_solution = x
            if callback_func is not None:
                if x is None:
                    x = x_of(state)
                callback_func(niter, x, energy1, energy2, elapsed, max_violated_equality, max_violated_inequality)
            state.dual_step()
            niter += 1
        else:
            k = min(nb_iter_plot - niter % nb_iter_plot, nb_max_iter - niter)
            state.iterate(k)
            niter += k
    return x_of(state), best_integer_solution


def close_device_cp(state):
    state.close()
    if getattr(state, "_owned", None) is not None:
        state._owned.close()
        state._owned = None


def chambolle_pock_ppd(
    c,
    a_eq,
    beq,
    a_ineq,
    b_lower,
    b_upper,
    lb,
    ub,
    x0=None,
    alpha=1,
    theta=1,
    nb_max_iter=100,
    callback_func=None,
    max_time=None,
    save_problem=False,
    force_integer=False,
    nb_iter_plot=10,
    order=ORDER_AUTO,
    setup="auto",
):
    """minimise c.x  s.t.  a_eq x = beq,  b_lower <= a_ineq x <= b_upper,  lb <= x <= ub.

    ``order`` (extension) selects the dot-product summation order, see
    include/slp_hip.h; the default reproduces the reference's iterates bit for
    bit while rows are short (mean <= 16 stored entries) and switches to
    wavefront-parallel sums for long rows.
    ``setup`` (extension): ``"host"`` stacks ``[A_eq; K_ineq]`` on the host and
    uploads it (reference :74-88,145-233); ``"device"`` uploads the two blocks
    as they are and stacks them on the device (``device_cp``); ``"auto"`` takes
    the device at ``SparseLP.DEVICE_SETUP_ENTRIES`` stored entries or more.
    """
    if save_problem or force_integer:
        # debugging pickle / rounding heuristic of the reference: outside the accelerated path
        raise NotImplementedError("save_problem / force_integer are not supported by pysparselp_amd")
    x, best_integer_solution, _, has_rows = _cp_run(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0, alpha, theta, nb_max_iter,
                                                    callback_func, max_time, nb_iter_plot, order, setup)
    return (x, best_integer_solution) if has_rows else x


def _gap_info(state):
    iterations, stopped, primal, bound, violation = state.gap_state()
    return dict(iterations=iterations, stopped=stopped, primal=primal, lower_bound=bound, violation=violation)


def _cp_run(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0, alpha, theta, nb_max_iter, callback_func, max_time, nb_iter_plot, order,
            setup, gap=None):
    """``chambolle_pock_ppd`` (``gap`` None) and ``chambolle_pock_ppd_certified`` (``gap`` the checked ``(tol_gap, tol_feas,
    check_every)``): ``(x, best_integer_solution, info, has_rows)``; ``info`` is None without a test; an LP without rows (``has_rows``
    False) ran nothing: ``x`` is its box vertex (which ``chambolle_pock_ppd`` returns alone, as the reference does, :147-151)."""
    start = time.perf_counter()
    c = _lib.f64(c)
    lb, ub = _lib.f64(lb), _lib.f64(ub)
    n = c.size
    assert lb.size == n and ub.size == n
    if a_eq is not None and a_eq.shape[0] == 0:  # reference :70-72
        a_eq, beq = None, None
    if a_ineq is not None and a_ineq.shape[0] == 0:
        a_ineq = None
    if a_eq is None and a_ineq is None:  # reference :147-151: no constraints, a vertex of the box
        x = box_vertex(c, lb, ub)
        return x, None, None if gap is None else vertex_certificate(c, x), False
    for a in (a_eq, a_ineq):
        if a is not None:
            assert a.shape[1] == n
    from . import host_setup

    info = None
    if host_setup.choose(setup, host_setup.nnz_of(a_eq, a_ineq)) == "device":
        state, _, _ = device_cp(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0, alpha, theta, order)
        try:
            if gap is not None:
                state.set_stop_gap(*gap)
            x, best_integer_solution = _cp_loop(state, c, n, a_ineq is not None, nb_max_iter, nb_iter_plot, callback_func, max_time,
                                                start, lambda st: st.x_reduced(), None if gap is None else lambda: state.gap_state()[1])
            if gap is not None:
                info = _gap_info(state)
        finally:
            close_device_cp(state)
        return x, best_integer_solution, info, True
    ineq, b_ineq = (None, None)
    if a_ineq is not None:
        ineq, b_ineq = one_sided_system(a_ineq, b_lower, b_upper)
        assert b_ineq.size == ineq[3]

    state = CPState(c, a_eq, beq, ineq, b_ineq, lb, ub, x0, alpha, theta, order)
    try:
        if gap is not None:
            state.set_stop_gap(*gap)
        x, best_integer_solution = _cp_loop(state, c, n, a_ineq is not None, nb_max_iter, nb_iter_plot, callback_func, max_time, start,
                                            lambda st: st.x(), None if gap is None else lambda: state.gap_state()[1])
        if gap is not None:
            info = _gap_info(state)
    finally:
        state.close()
    if best_integer_solution is not None:
        best_integer_solution = best_integer_solution[:n]
    return x[:n], best_integer_solution, info, True


def chambolle_pock_ppd_certified(
    c,
    a_eq,
    beq,
    a_ineq,
    b_lower,
    b_upper,
    lb,
    ub,
    tol_gap,
    tol_feas,
    check_every=10,
    x0=None,
    alpha=1,
    theta=1,
    nb_max_iter=10000,
    callback_func=None,
    max_time=None,
    nb_iter_plot=10,
    order=ORDER_AUTO,
    setup="auto",
):
    """``chambolle_pock_ppd`` that stops on a certificate (extension; the reference stops on nothing): at the first iteration
    ``t`` with ``t % check_every == 0`` at which the violation of ``x_t`` is at most ``tol_feas`` and the gap between ``c.x_t``
    and a valid lower bound is at most ``tol_gap * (1 + |primal| + |bound|)`` (``CPState.set_stop_gap``), or after
    ``nb_max_iter`` iterations.  Every format and set-up of ``chambolle_pock_ppd``, and its row partition under a communicator.

    Returns ``(x, best_integer_solution, info)``; ``info`` is a dict of ``iterations`` (whole iterations completed), ``stopped``,
    and the last evaluated certificate ``primal``, ``lower_bound``, ``violation`` of the LP the solver holds (``+inf``, ``-inf``,
    ``+inf`` before the first check).  ``x`` is bit for bit ``chambolle_pock_ppd(..., nb_max_iter=info["iterations"])[0]``.  The
    reporting loop is that of ``chambolle_pock_ppd``; it ends, without a report, at the first report that finds the state
    stopped.  ``tol_gap`` and ``tol_feas`` finite floats ``>= 0`` and ``check_every`` an int ``>= 1``: a ``ValueError`` otherwise,
    before anything is uploaded.  An LP without rows returns its box vertex, stopped after 0 iterations, with that vertex's
    certificate."""
    gap = check_gap(tol_gap, tol_feas, check_every)
    return _cp_run(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0, alpha, theta, nb_max_iter, callback_func, max_time, nb_iter_plot,
                   order, setup, gap)[:3]


# ---------------------------------------------------------------------------------------------------------------------
# batched form: B LPs over one constraint structure
def one_sided_system_batch(a_ineq, b_lower, b_upper):
    """``one_sided_system`` for right-hand sides that may carry a leading instance axis: the row selection (which bounds are
    finite, reference :74-88) must be the same for every instance -- ``ValueError`` otherwise --, the structure is that of
    ``one_sided_system`` and the selection is applied to every instance's bounds.  Returns ``(mat, b)``, ``b`` of shape
    ``(rows,)`` when both bounds are shared, else ``(B, rows)``."""
    b_upper = np.asarray(b_upper, dtype=np.float64)
    lower = None if b_lower is None else np.asarray(b_lower, dtype=np.float64)
    if b_upper.ndim == 1 and (lower is None or lower.ndim == 1):
        return one_sided_system(a_ineq, lower, b_upper)
    batch = b_upper.shape[0] if b_upper.ndim == 2 else lower.shape[0]
    bu = np.broadcast_to(b_upper, (batch, b_upper.shape[-1]))
    if lower is None:
        # (as the reference: without b_lower no row is selected, infinite upper bounds stay)
        mat, _ = one_sided_system(a_ineq, None, bu[0])
        return mat, np.ascontiguousarray(bu)
    bl = np.broadcast_to(lower, (batch, lower.shape[-1]))
    up_mask, lo_mask = bu != np.inf, bl != -np.inf
    if np.any(up_mask != up_mask[0]) or np.any(lo_mask != lo_mask[0]):
        k = int(np.nonzero(np.any(up_mask != up_mask[0], axis=1) | np.any(lo_mask != lo_mask[0], axis=1))[0][0])
        raise ValueError(f"instance {k} has another pattern of finite b_lower / b_upper than instance 0: the one-sided stacking "
                         "(which rows exist) must be the same for all instances of a batch")
    mat, _ = one_sided_system(a_ineq, bl[0], bu[0])
    up, lo = np.nonzero(up_mask[0])[0], np.nonzero(lo_mask[0])[0]
    return mat, np.ascontiguousarray(np.hstack((bu[:, up], -bl[:, lo])))


class CPBatchState:
    """Device-resident batched Chambolle-Pock state (thin RAII wrapper of ``slp_cp_batch``): ``c`` is ``(B, n)``; ``beq``,
    ``b_ineq``, ``lb``, ``ub``, ``x0`` are shared vectors or carry a leading axis ``B``; ``ineq`` as ``CPState``'s."""

    def __init__(self, c, a_eq, beq, ineq, b_ineq, lb, ub, x0, alpha, theta):
        c = _lib.f64(c)
        if c.ndim != 2 or c.shape[0] < 1:
            raise ValueError(f"c has shape {c.shape}: expected (B, n) with B >= 1")
        self.batch, self.n = c.shape
        lb, lb_b = shared_or_batched("lb", lb, self.batch, self.n)
        ub, ub_b = shared_or_batched("ub", ub, self.batch, self.n)
        x0, x0_b = (None, False) if x0 is None else shared_or_batched("x0", x0, self.batch, self.n)
        parts_ptr, parts_idx, parts_val, parts_b = [np.zeros(1, dtype=np.int64)], [], [], []
        self.m_eq = 0
        if a_eq is not None:
            p, j, v = _lib.csr_arrays(a_eq)
            self.m_eq = a_eq.shape[0]
            parts_ptr.append(p[1:])
            parts_idx.append(j)
            parts_val.append(v)
            parts_b.append(shared_or_batched("beq", beq, self.batch, self.m_eq))
        self.m_ineq = 0
        if ineq is not None:
            p, j, v, rows = ineq
            self.m_ineq = rows
            off = parts_ptr[-1][-1] if len(parts_ptr) > 1 else 0
            parts_ptr.append(off + p[1:])
            parts_idx.append(j)
            parts_val.append(v)
            parts_b.append(shared_or_batched("b_ineq", b_ineq, self.batch, rows))
        indptr = np.ascontiguousarray(np.concatenate(parts_ptr), dtype=np.int64)
        indices = np.ascontiguousarray(np.concatenate(parts_idx) if parts_idx else np.zeros(0), dtype=np.int32)
        data = _lib.f64(np.concatenate(parts_val) if parts_val else np.zeros(0))
        if indices.size and (indices.min() < 0 or indices.max() >= self.n):
            raise ValueError("constraint matrix has a column index outside [0, n)")
        if self.m_eq + self.m_ineq == 0:
            raise ValueError("no constraint rows: chambolle_pock_ppd_batch returns the box vertex without a solver state")
        b_b = any(flag for _, flag in parts_b)
        if b_b:  # one kind of rows shared, the other per instance: the shared part is replicated here
            b = np.ascontiguousarray(np.hstack([v if flag else np.broadcast_to(v, (self.batch, v.size)) for v, flag in parts_b]))
        else:
            b = np.ascontiguousarray(np.concatenate([v for v, _ in parts_b]))
        # all of the above needs no GPU; the library is loaded (and bound to a device) only now
        self._l = _lib.lib()
        self._h = _lib.check_handle(self._l.slp_cp_batch_create(
            self.n, self.m_eq, self.m_ineq, _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(data), self.batch, _lib.ptr(b), int(b_b),
            _lib.ptr(c), _lib.ptr(lb), int(lb_b), _lib.ptr(ub), int(ub_b), _lib.ptr(x0), int(x0_b), float(alpha), float(theta)))

    def close(self):
        if getattr(self, "_h", None):
            self._l.slp_cp_batch_destroy(self._h)
            self._h = None

    __del__ = close

    def iterate(self, k):
        _lib.check(self._l.slp_cp_batch_iterate(self._h, int(k)))

    def primal_step(self):
        _lib.check(self._l.slp_cp_batch_primal_step(self._h))

    def dual_step(self):
        _lib.check(self._l.slp_cp_batch_dual_step(self._h))

    def report(self):
        """``(B, 5)``: energy1, energy2, max |A_e z - b_e|, max (A_i x - b_i), max |A_e x - b_e| per instance."""
        out = np.zeros((self.batch, 5))
        _lib.check(self._l.slp_cp_batch_report(self._h, _lib.ptr(out)))
        return out

    def x(self):
        out = np.empty((self.batch, self.n))
        _lib.check(self._l.slp_cp_batch_get_x(self._h, _lib.ptr(out)))
        return out

    def y(self):
        out = np.empty((self.batch, self.m_eq + self.m_ineq))
        _lib.check(self._l.slp_cp_batch_get_y(self._h, _lib.ptr(out)))
        return out

    def preconditioners(self):
        t, s = np.empty(self.n), np.empty(self.m_eq + self.m_ineq)
        _lib.check(self._l.slp_cp_batch_get_preconditioners(self._h, _lib.ptr(t), _lib.ptr(s)))
        return t, s

    def bench(self, k):
        ms = np.zeros(3)
        _lib.check(self._l.slp_cp_batch_bench(self._h, int(k), _lib.ptr(ms)))
        return ms

    def set_stop_gap(self, tol_gap, tol_feas, check_every=1):
        """Arms the certificate as the per-instance stopping test (``slp_cp_batch_set_stop_gap``, include/slp_hip_ext.h); the
        certificate is that of ``CPManyState.set_stop_gap``.  The state counts its whole iterations ``t`` from 1 over its life,
        those before the arming included.  At the end of every iteration ``t`` with ``t % check_every == 0`` each running instance
        evaluates, for the LP the solver holds (``K = [A_eq; A_ineq]`` one-sided, ``y_t`` the clamped multipliers), ``primal =
        c.x_t``, the lower bound ``sum_j min(d_j lb_j, d_j ub_j) - y_t.b`` with ``d = c + K^T y_t`` (terms with ``d_j == 0`` or ``y_r
        == 0`` left out; ``-inf`` where a free variable has ``d_j`` of the wrong sign) and ``violation = max(max|A_eq x_t - b_eq|,
        max(A_ineq x_t - b_ineq), 0)``; it stops iff ``violation <= tol_feas`` and ``|primal - bound| <= tol_gap * (1 + |primal| +
        |bound|)`` with a finite left-hand side.  A NaN never stops.  A stopped instance keeps its iterate -- bit for bit that of
        the batch without a test after as many iterations -- while the others go on.

        Unlike an LP of a list, a stopped instance STAYS stopped for the life of the state: the batch has one iteration counter.
        Calling this again changes the tolerances and the cadence for the running instances and keeps the flags.  ``tol_gap=None``
        disarms: the running instances go on untested, the stopped ones stay frozen.  Once every instance is stopped ``iterate``
        and ``dual_step`` do nothing and the count of iterations stays.  Between whole iterations only."""
        if tol_gap is None:
            tol_gap, tol_feas, check_every = -1.0, 0.0, 1
        else:
            tol_gap, check_every = _many.check_stop(tol_gap, check_every, "tol_gap")
            tol_feas, _ = _many.check_stop(tol_feas, check_every, "tol_feas")
        _lib.check(self._l.slp_cp_batch_set_stop_gap(self._h, tol_gap, tol_feas, check_every))

    def gap_state(self):
        """``(iterations, stopped, primal, bound, violation)`` per instance, int64, bool and three float64 arrays: the iterations
        completed (for a stopped instance its stopping iteration), whether it is stopped, and the numbers of the last evaluated
        certificate (``+inf``, ``-inf``, ``+inf`` before the first).  A stopped instance stays stopped for the life of the state."""
        iterations, stopped = np.zeros(self.batch, dtype=np.int64), np.zeros(self.batch, dtype=np.int32)
        primal, bound, violation = np.zeros(self.batch), np.zeros(self.batch), np.zeros(self.batch)
        _lib.check(self._l.slp_cp_batch_gap_state(self._h, _lib.ptr(iterations), _lib.ptr(stopped), _lib.ptr(primal), _lib.ptr(bound),
                                                  _lib.ptr(violation)))
        return iterations, stopped.astype(bool), primal, bound, violation


def _cp_report_loop(state, costs, has_ineq, slots, best, all_x, spread, nb_max_iter, nb_iter_plot, callback_func, max_time, start,
                    stopped_now=None):
    """``_cp_loop`` for a batched or a list state: same cadence; the report's numbers are arrays with one entry per LP of the
    state, ``max_time`` stops them all.  ``costs[i]`` and ``has_ineq[i]`` belong to the state's LP ``i``; its best feasible iterate
    (:284-291 with force_integer=False) goes to ``best[slots[i]]``.  ``all_x`` and ``spread(values, energy=False)`` map the
    state's iterates and numbers to what the callback sees: the identity for a batch, the whole list (LPs without rows
    included) for a list.  Returns ``all_x`` of the final iterates.

    ``stopped_now()`` (a state with a per-LP stopping test; ``None``: none) is asked before every report which of the state's LPs
    are stopped, a bool array: when all are, the loop ends there, without a report; else a stopped LP's five numbers repeat the
    last row it had while it was running, and it is no candidate for ``best`` any more."""
    best_energy = np.full(len(slots), np.inf)
    niter = 0
    last = None
    while niter < nb_max_iter:
        if niter % nb_iter_plot == 0:
            stopped = None if stopped_now is None else stopped_now()
            if stopped is not None and stopped.all():
                break
            state.primal_step()
            elapsed = time.perf_counter() - start
            if (max_time is not None) and collective_elapsed(elapsed) > max_time:  # the same decision on every rank
                break
            numbers = state.report()
            if stopped is not None:
                if last is not None:
                    numbers[stopped] = last[stopped]
                last = numbers
            energy1, energy2, max_violated_equality, max_violated_inequality, max_eq_at_x = numbers.T.copy()
            max_violated_inequality[~has_ineq] = 0  # the reference dereferences a_ineq here (:283) and fails
            x = None
            feasible = (max_eq_at_x == 0) & (max_violated_inequality <= 0)
            if stopped is not None:
                feasible &= ~stopped
            feasible = np.nonzero(feasible)[0]
            if feasible.size:
                x = state.x()
                for i in feasible:
                    energy_rounded = costs[i].dot(x[i])
                    if energy_rounded < best_energy[i]:
                        best_energy[i] = energy_rounded
                        best[slots[i]] = x[i].copy()
            if callback_func is not None:
                if x is None:
                    x = state.x()
                callback_func(niter, all_x(x), spread(energy1, True), spread(energy2, True), elapsed, spread(max_violated_equality),
                              spread(max_violated_inequality))
            state.dual_step()
            niter += 1
        else:
            k = min(nb_iter_plot - niter % nb_iter_plot, nb_max_iter - niter)
            state.iterate(k)
            niter += k
    return all_x(state.x())


def chambolle_pock_ppd_batch(
    c,
    a_eq,
    beq,
    a_ineq,
    b_lower,
    b_upper,
    lb,
    ub,
    x0=None,
    alpha=1,
    theta=1,
    nb_max_iter=100,
    callback_func=None,
    max_time=None,
    nb_iter_plot=10,
):
    """``chambolle_pock_ppd`` for B LPs at once (extension; the reference solves one LP per call):
    minimise ``c[k].x``  s.t.  ``a_eq x = beq[k]``, ``b_lower[k] <= a_ineq x <= b_upper[k]``, ``lb[k] <= x <= ub[k]`` for every k.

    ``c`` has shape ``(B, n)``; ``beq``, ``b_lower``, ``b_upper``, ``lb``, ``ub``, ``x0`` each have their single-instance shape
    (shared by all instances) or a leading axis ``B``.  The instances share the constraint matrices, hence the one-sided
    stacking (:74-88): which of ``b_lower`` / ``b_upper`` are finite must be the same for every instance (``ValueError``
    otherwise, like every shape error raised before anything is uploaded).  All B iterates advance in the same two launches
    per iteration; every instance is bit for bit what ``chambolle_pock_ppd(..., order=ORDER_SEQUENTIAL)`` computes for it.

    The reporting loop is that of ``chambolle_pock_ppd``: ``callback_func(niter, X, energy1, energy2, elapsed,
    max_violated_equality, max_violated_inequality)`` every ``nb_iter_plot`` iterations with ``X`` of shape ``(B, n)`` and arrays
    of length B; ``max_time`` stops the whole batch at a report.  Returns ``(X, best_integer_solutions)``, the latter a list
    of B entries (``None`` or the best feasible iterate of that instance, :284-291).  Without any constraint it returns the
    box vertex of every instance, ``X`` alone, as the reference does (:147-151).

    Under a communicator every rank solves the whole batch (a replica): the rows are not partitioned.
    """
    x, best, _ = _cp_batch_run(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0, alpha, theta, nb_max_iter, callback_func, max_time,
                               nb_iter_plot)
    return x if best is None else (x, best)


def _cp_batch_run(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0, alpha, theta, nb_max_iter, callback_func, max_time, nb_iter_plot,
                  gap=None):
    """``chambolle_pock_ppd_batch`` (``gap`` None) and ``chambolle_pock_ppd_batch_certified`` (``gap`` the checked ``(tol_gap,
    tol_feas, check_every)``): ``(X, best_integer_solutions, info)``; ``best_integer_solutions`` is None for a batch without
    constraint rows, ``info`` None without a stopping test."""
    start = time.perf_counter()
    c = np.asarray(c, dtype=np.float64)
    if c.ndim != 2:
        raise ValueError(f"c has shape {c.shape}: expected (B, n), one row of costs per instance")
    batch, n = c.shape
    if batch < 1:
        raise ValueError("an empty batch: c needs at least one row (B >= 1)")
    c = np.ascontiguousarray(c)
    lb, _ = shared_or_batched("lb", lb, batch, n)
    ub, _ = shared_or_batched("ub", ub, batch, n)
    if x0 is not None:
        x0, _ = shared_or_batched("x0", x0, batch, n)
    if a_eq is not None and a_eq.shape[0] == 0:  # reference :70-72
        a_eq, beq = None, None
    if a_ineq is not None and a_ineq.shape[0] == 0:
        a_ineq = None
    for name, a in (("a_eq", a_eq), ("a_ineq", a_ineq)):
        if a is not None:
            if a.shape[1] != n:
                raise ValueError(f"{name} has {a.shape[1]} columns, c has {n}")
            if a.indices.size and (a.indices.min() < 0 or a.indices.max() >= n):
                raise ValueError(f"{name} has a column index outside [0, {n})")
    if a_eq is not None:
        beq, _ = shared_or_batched("beq", beq, batch, a_eq.shape[0])
    if a_eq is None and a_ineq is None:  # reference :147-151: no constraints, a vertex of the box per instance
        x = box_vertex(c, lb, ub)
        info = None
        if gap is not None:   # the vertex is optimal: primal and bound are its value
            value = np.array([c[k].dot(x[k]) for k in range(batch)])
            info = dict(iterations=np.zeros(batch, dtype=np.int64), stopped=np.ones(batch, dtype=bool), primal=value,
                        lower_bound=value.copy(), violation=np.zeros(batch))
        return x, None, info
    ineq, b_ineq = (None, None)
    if a_ineq is not None:
        rows = a_ineq.shape[0]
        b_upper, _ = shared_or_batched("b_upper", b_upper, batch, rows)
        if b_lower is not None:
            b_lower, _ = shared_or_batched("b_lower", b_lower, batch, rows)
        ineq, b_ineq = one_sided_system_batch(a_ineq, b_lower, b_upper)
        assert b_ineq.shape[-1] == ineq[3]

    info = None
    if gap is not None:
        info = dict(iterations=np.zeros(batch, dtype=np.int64), stopped=np.zeros(batch, dtype=bool), primal=np.full(batch, np.inf),
                    lower_bound=np.full(batch, -np.inf), violation=np.full(batch, np.inf))
    state = CPBatchState(c, a_eq, beq, ineq, b_ineq, lb, ub, x0, alpha, theta)
    best = [None] * batch

    def stopped_now():
        now = state.gap_state()
        for name, values in zip(_GAP_INFO, now):
            info[name][:] = values
        return now[1]

    try:
        if gap is not None:
            state.set_stop_gap(*gap)
            if callback_func is not None:
                try:
                    callback_func.info = info
                except AttributeError:   # a bound method takes no attribute: wrap it in a function to read ``info``
                    pass
        x = _cp_report_loop(state, c, np.full(batch, a_ineq is not None), range(batch), best, lambda x: x,
                            lambda values, energy=False: values, nb_max_iter, nb_iter_plot, callback_func, max_time, start,
                            None if gap is None else stopped_now)
        if gap is not None:
            stopped_now()
    finally:
        state.close()
    return x, best, info


def chambolle_pock_ppd_batch_certified(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, tol_gap, tol_feas, check_every=10, x0=None,
                                       alpha=1, theta=1, nb_max_iter=10000, callback_func=None, max_time=None, nb_iter_plot=10):
    """``chambolle_pock_ppd_batch`` with a certificate as the stopping test per instance (extension; the reference evaluates the
    same lower bound, its ``energy2``, at its reports and stops on nothing): the batch runs until every instance has stopped, at
    most ``nb_max_iter`` iterations.  Returns ``(X, best_integer_solutions, info)``.

    The test is that of ``chambolle_pock_ppd_many_certified``, made on the device after the dual half of every iteration ``t``
    with ``t % check_every == 0``, iterations counted from 1 (``CPBatchState.set_stop_gap``), on the LP the solver holds: with
    ``primal = c[k].x_t``, ``lower_bound = sum_j min(d_j lb_j, d_j ub_j) - y_t.b`` for ``d = c[k] + K^T y_t`` and ``violation =
    max(max|A_eq x_t - b_eq|, max(A_ineq x_t - b_ineq), 0)`` instance ``k`` stops iff ``violation <= tol_feas`` and ``|primal -
    lower_bound| <= tol_gap * (1 + |primal| + |lower_bound|)`` with a finite left-hand side; an instance with a lower bound of
    ``-inf`` or a NaN does not stop.  A stopped instance keeps its iterate after ``t`` iterations, bit for bit that of
    ``chambolle_pock_ppd(..., nb_max_iter=t, order=ORDER_SEQUENTIAL)``, while the others go on; it stays stopped.  ``tol_gap`` and
    ``tol_feas`` are finite floats ``>= 0``, ``check_every`` an int ``>= 1``: a ``ValueError`` before the library is loaded
    otherwise, like every shape error.

    ``info`` is a dict of arrays of length B: ``iterations`` (int64: completed, for a stopped instance its stopping iteration),
    ``stopped`` (bool), and ``primal``, ``lower_bound``, ``violation`` (float64: the last evaluated certificate; ``+inf``, ``-inf``,
    ``+inf`` before the first).  The two sums are in the device's own fixed order.  Without any constraint row every instance is
    stopped after 0 iterations at its box vertex: ``primal`` and ``lower_bound`` are both its cost, ``violation`` is 0 and
    ``best_integer_solutions`` is a list of ``None``.

    Reports, callbacks, ``callback_func.info`` (the same dict, updated in place, current at every callback) and the end of the
    loop are those of ``chambolle_pock_ppd_many_until``: the loop ends at the first report index at which every instance is
    stopped, at ``nb_max_iter``, or at ``max_time``; a stopped instance's five numbers repeat the last row it had while it ran.
    """
    tol_gap, every = _many.check_stop(tol_gap, check_every, "tol_gap")
    tol_feas, _ = _many.check_stop(tol_feas, check_every, "tol_feas")
    x, best, info = _cp_batch_run(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0, alpha, theta, nb_max_iter, callback_func, max_time,
                                  nb_iter_plot, (tol_gap, tol_feas, every))
    return x, ([None] * x.shape[0] if best is None else best), info


# ---------------------------------------------------------------------------------------------------------------------
# a set of LPs with different matrices: one workgroup per LP
def _many_problem(k, problem):
    """LP ``k`` of a set, validated (``ValueError``) and brought to the solver's form without touching the library:
    ``(c, lb, ub, eq, beq, ineq, b_ineq)`` with ``eq`` raw CSR arrays ``(indptr, indices, data, rows)`` or ``None``, ``ineq`` the
    one-sided system of ``one_sided_system`` or ``None``."""
    c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub = _many.unpack_problem(k, problem)
    c = _many.check_cost(k, "c", c)
    n = c.size
    lb, ub = (_many.check_vector(k, name, v, (n,), f"c has {n} entries") for name, v in (("lb", lb), ("ub", ub)))
    if a_eq is not None and a_eq.shape[0] == 0:  # reference :70-72
        a_eq, beq = None, None
    if a_ineq is not None and a_ineq.shape[0] == 0:
        a_ineq = None
    for name, a in (("a_eq", a_eq), ("a_ineq", a_ineq)):
        if a is not None:
            _many.check_csr(k, name, a, n, f"c has {n} entries")
    eq = None
    if a_eq is not None:
        beq = _many.check_vector(k, "beq", beq, (a_eq.shape[0],), f"a_eq has {a_eq.shape[0]} rows")
        eq = _lib.csr_arrays(a_eq) + (a_eq.shape[0],)
    ineq, b_ineq = None, None
    if a_ineq is not None:
        rows = a_ineq.shape[0]
        b_upper = _many.check_vector(k, "b_upper", b_upper, (rows,), f"a_ineq has {rows} rows")
        if b_lower is not None:
            b_lower = _many.check_vector(k, "b_lower", b_lower, (rows,), f"a_ineq has {rows} rows")
        ineq, b_ineq = one_sided_system(a_ineq, b_lower, b_upper)
    return c, lb, ub, eq, beq, ineq, b_ineq


def many_system(lps):
    """The LPs ``(c, lb, ub, eq, beq, ineq, b_ineq)`` of ``_many_problem`` (each with at least one row) as the one system
    ``slp_cp_many_create`` takes -- a dict of:

    ``n``, ``m_eq``, ``m_ineq``: the shapes, int64 arrays of length ``count``;
    ``col0``, ``eq0``, ``in0``: the per-LP table -- first column, first equality row and first inequality row of every LP;
    ``indptr``, ``indices``, ``data``: the block-diagonal CSR of the ``K_k = [A_eq,k; A_ineq,k]``: the columns of LP k offset by
    ``col0[k]``; the rows are the equality rows of all LPs (LP 0, LP 1, ...) followed by the inequality rows of all LPs;
    ``b`` in that row order; ``c``, ``lb``, ``ub`` concatenated LP by LP."""
    count = len(lps)
    n = np.array([lp[0].size for lp in lps], dtype=np.int64)
    m_eq = np.array([0 if lp[3] is None else lp[3][3] for lp in lps], dtype=np.int64)
    m_ineq = np.array([0 if lp[5] is None else lp[5][3] for lp in lps], dtype=np.int64)
    col0, eq0 = first_offsets(n), first_offsets(m_eq)
    in0 = int(m_eq.sum()) + first_offsets(m_ineq)
    if int(n.sum()) >= 2 ** 31 or int(m_eq.sum() + m_ineq.sum()) >= 2 ** 31:
        raise ValueError("the set has 2^31 or more variables or rows")
    # (LP, its block, its right-hand side): the equality rows of all LPs, then the inequality rows of all LPs
    rows = [(k, lps[k][part], lps[k][rhs]) for part, rhs in ((3, 4), (5, 6)) for k in range(count) if lps[k][part] is not None]
    indptr, indices, data = _many.stack_blocks([a[:3] for _, a, _ in rows], [col0[k] for k, _, _ in rows])
    return dict(n=n, m_eq=m_eq, m_ineq=m_ineq, col0=col0, eq0=eq0, in0=in0, indptr=indptr, indices=indices, data=data,
                b=concat([b for _, _, b in rows], np.float64), c=concat([lp[0] for lp in lps], np.float64),
                lb=concat([lp[1] for lp in lps], np.float64), ub=concat([lp[2] for lp in lps], np.float64))


class CPManyState(_many.ManyState):
    """Device-resident Chambolle-Pock state of a set of LPs (thin RAII wrapper of ``slp_cp_many``).  ``lps``: the LPs as
    ``_many_problem`` returns them, each with at least one row; ``x0``: ``None`` or one start (or ``None``: zeros) per LP."""

    _PREFIX = "slp_cp_many"
    _LIVE = "slp_many_cp"

    def __init__(self, lps, x0=None, alpha=1, theta=1):
        if len(lps) < 1:
            raise ValueError("an empty set of LPs")
        s = many_system(lps)
        self.count = len(lps)
        self.n, self.m = s["n"], s["m_eq"] + s["m_ineq"]
        self.system = s
        start = _many.concat_starts(x0, self.n)
        # all of the above needs no GPU; the library is loaded (and bound to a device) only now
        self._l = _lib.lib()
        self._h = _lib.check_handle(self._l.slp_cp_many_create(
            self.count, _lib.ptr(s["n"]), _lib.ptr(s["m_eq"]), _lib.ptr(s["m_ineq"]), _lib.ptr(s["indptr"]), _lib.ptr(s["indices"]),
            _lib.ptr(s["data"]), _lib.ptr(s["b"]), _lib.ptr(s["c"]), _lib.ptr(s["lb"]), _lib.ptr(s["ub"]), _lib.ptr(start),
            float(alpha), float(theta)))

    def iterate(self, k):
        _lib.check(self._l.slp_cp_many_iterate(self._h, int(k)))

    def primal_step(self):
        _lib.check(self._l.slp_cp_many_primal_step(self._h))

    def dual_step(self):
        _lib.check(self._l.slp_cp_many_dual_step(self._h))

    def report(self):
        """``(count, 5)``: energy1, energy2, max |A_e z - b_e|, max (A_i x - b_i), max |A_e x - b_e| per LP."""
        out = np.zeros((self.count, 5))
        _lib.check(self._l.slp_cp_many_report(self._h, _lib.ptr(out)))
        return out

    def set_stop(self, tol, check_every=1):
        """Arms the per-LP stopping test of the iteration kernel (``slp_many_cp_set_stop``): at the end of every iteration ``t``
        of an LP with ``t % check_every == 0`` -- counted from 1 over the LP's life -- the LP stops iff ``max(max|x_t - x_{t-1}|,
        max|y_t - y_{t-1}|) <= tol``; a stopped LP keeps its iterate and takes no part in later calls.  ``tol=None`` turns the test
        off, the state after the constructor.  Between whole iterations only.  Every call clears the stopped flags and keeps the
        counters."""
        if tol is None:
            tol, check_every = -1.0, 1
        else:
            tol, check_every = _many.check_stop(tol, check_every)
        _lib.check(self._l.slp_many_cp_set_stop(self._h, tol, check_every))

    def stop_state(self):
        """``(iterations, stopped, step)`` per LP, int64, bool and float64 arrays: the iterations completed (for a stopped LP its
        stopping iteration), whether it is stopped and the last evaluated step (``+inf`` before the first test)."""
        iterations, stopped, step = np.zeros(self.count, dtype=np.int64), np.zeros(self.count, dtype=np.int32), np.zeros(self.count)
        _lib.check(self._l.slp_many_cp_stop_state(self._h, _lib.ptr(iterations), _lib.ptr(stopped), _lib.ptr(step)))
        return iterations, stopped.astype(bool), step

    def set_stop_gap(self, tol_gap, tol_feas, check_every=1):
        """Arms the certificate as the per-LP stopping test of the iteration kernel (``slp_many_cpgap_set_stop``) and disarms the
        step test of ``set_stop``: at the end of every iteration ``t`` of an LP with ``t % check_every == 0`` -- counted from 1
        over the LP's life -- the kernel evaluates, for the LP the solver holds (``K = [A_eq; A_ineq]`` one-sided, ``y_t`` the
        clamped multipliers), ``primal = c.x_t``, the lower bound ``sum_j min(d_j lb_j, d_j ub_j) - y_t.b`` with ``d = c + K^T
        y_t`` (terms with ``d_j == 0`` or ``y_r == 0`` left out; ``-inf`` where a free variable has ``d_j`` of the wrong sign) and
        ``violation = max(max|A_eq x_t - b_eq|, max(A_ineq x_t - b_ineq), 0)``; the LP stops iff ``violation <= tol_feas`` and
        ``|primal - bound| <= tol_gap * (1 + |primal| + |bound|)`` with a finite left-hand side.  A NaN never stops.  A stopped LP
        keeps its iterate and takes no part in later calls.  ``tol_gap=None`` turns the test off.  Between whole iterations only.
        Every call clears the stopped flags and keeps the counters."""
        if tol_gap is None:
            tol_gap, tol_feas, check_every = -1.0, 0.0, 1
        else:
            tol_gap, check_every = _many.check_stop(tol_gap, check_every, "tol_gap")
            tol_feas, _ = _many.check_stop(tol_feas, check_every, "tol_feas")
        _lib.check(self._l.slp_many_cpgap_set_stop(self._h, tol_gap, tol_feas, check_every))

    def gap_state(self):
        """``(iterations, stopped, primal, bound, violation)`` per LP, int64, bool and three float64 arrays: the iterations
        completed (for a stopped LP its stopping iteration), whether it is stopped, and the numbers of the last evaluated
        certificate (``+inf``, ``-inf``, ``+inf`` before the first)."""
        iterations, stopped = np.zeros(self.count, dtype=np.int64), np.zeros(self.count, dtype=np.int32)
        primal, bound, violation = np.zeros(self.count), np.zeros(self.count), np.zeros(self.count)
        _lib.check(self._l.slp_many_cpgap_state(self._h, _lib.ptr(iterations), _lib.ptr(stopped), _lib.ptr(primal), _lib.ptr(bound),
                                                 _lib.ptr(violation)))
        return iterations, stopped.astype(bool), primal, bound, violation

    def x(self):
        return self._per_lp("x", self.n)

    def y(self):
        """Per LP ``[y_eq; y_ineq]``."""
        return self._per_lp("y", self.m)

    def preconditioners(self):
        t, s = np.empty(int(self.n.sum())), np.empty(int(self.m.sum()))
        _lib.check(self._l.slp_cp_many_get_preconditioners(self._h, _lib.ptr(t), _lib.ptr(s)))
        return split_by(t, self.n), split_by(s, self.m)

    def bench(self, k):
        ms = np.zeros(3)
        _lib.check(self._l.slp_cp_many_bench(self._h, int(k), _lib.ptr(ms)))
        return ms


def many_lds_limit():
    """Doubles of x, z, y (``2 n + m``) an LP may hold in LDS (``slp_cp_many_lds_limit``)."""
    return int(_lib.load().slp_cp_many_lds_limit())


def chambolle_pock_ppd_many(problems, x0=None, alpha=1, theta=1, nb_max_iter=100, callback_func=None, max_time=None, nb_iter_plot=10):
    """``chambolle_pock_ppd`` for a list of LPs whose matrices differ (extension; the reference solves one LP per call).

    ``problems`` is a sequence of 8-tuples ``(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub)``, each as ``chambolle_pock_ppd``
    takes them (one-sided stacking for a finite ``b_lower``, :74-88; an absent kind of rows is ``None`` or a matrix without
    rows); ``x0`` is ``None`` or a sequence with one start (or ``None``) per LP; ``alpha`` and ``theta`` are shared.  Every shape
    error is a ``ValueError`` raised before the library is loaded.  The LPs become one block-diagonal system on the device and
    every LP is one workgroup that runs whole iterations inside one launch, its iterates in LDS where they fit
    (pysparselp_amd/csrc/slp_cp_many.hip); every LP is bit for bit what ``chambolle_pock_ppd(..., order=ORDER_SEQUENTIAL)``
    computes for it alone.

    The reporting loop is that of ``chambolle_pock_ppd``: ``callback_func(niter, xs, energy1, energy2, elapsed,
    max_violated_equality, max_violated_inequality)`` every ``nb_iter_plot`` iterations with ``xs`` a list of arrays and the rest
    arrays of length ``count``; ``max_time`` stops all LPs at a report.  Returns ``(xs, best_integer_solutions)``, two lists (the
    latter: ``None`` or the best feasible iterate of that LP, :284-291).  An LP without any constraint gets its box vertex
    (:147-151) and takes no part in the iterations.

    Under a communicator every rank solves the whole list (a replica).  For LPs that share one matrix
    ``chambolle_pock_ppd_batch`` reads the matrix once for all of them.  The block-diagonal concatenation of the list handed to
    ``chambolle_pock_ppd`` as ONE LP computes the same bits per block in two launches per iteration; which of the two is faster at
    a given count is what ``tools/bench_cp_many.py`` measures -- not measured yet.
    """
    xs, best, _ = _cp_many_run(problems, x0, alpha, theta, nb_max_iter, callback_func, max_time, nb_iter_plot, None)
    return xs, best


_GAP_INFO = ("iterations", "stopped", "primal", "lower_bound", "violation")


def _cp_many_run(problems, x0, alpha, theta, nb_max_iter, callback_func, max_time, nb_iter_plot, stop, gap=None):
    """``chambolle_pock_ppd_many`` (``stop`` and ``gap`` None), ``chambolle_pock_ppd_many_until`` (``stop`` the checked ``(tol,
    check_every)``) and ``chambolle_pock_ppd_many_certified`` (``gap`` the checked ``(tol_gap, tol_feas, check_every)``): ``(xs,
    best_integer_solutions, info)``, ``info`` None without a stopping test."""
    start = time.perf_counter()
    count = _many.count_problems(problems)
    lps = [_many_problem(k, p) for k, p in enumerate(problems)]
    x0 = _many.check_starts(x0, lps)
    solved = [k for k in range(count) if lps[k][3] is not None or lps[k][5] is not None]
    xs = [None if (lps[k][3] is not None or lps[k][5] is not None) else box_vertex(*lps[k][:3]) for k in range(count)]
    best = [None] * count
    free_energy = np.array([0.0 if xs[k] is None else lps[k][0].dot(xs[k]) for k in range(count)])
    info = None if stop is None else _many.new_stop_info(count, solved)
    if gap is not None:   # an LP without rows: its vertex is optimal, primal and bound are its value
        info = dict(iterations=np.zeros(count, dtype=np.int64), stopped=np.ones(count, dtype=bool), primal=free_energy.copy(),
                    lower_bound=free_energy.copy(), violation=np.zeros(count))
        info["stopped"][solved] = False
        info["primal"][solved] = info["violation"][solved] = np.inf
        info["lower_bound"][solved] = -np.inf
    if not solved:
        return xs, best, info
    costs = [lps[k][0] for k in solved]
    has_ineq = np.array([lps[k][5] is not None for k in solved])
    state = CPManyState([lps[k] for k in solved], None if x0 is None else [x0[k] for k in solved], alpha, theta)

    def spread(values, energy=False):
        """Per-LP numbers of the solved LPs over the whole list."""
        out = free_energy.copy() if energy else np.zeros(count)
        out[solved] = values
        return out

    def all_x(part):
        out = list(xs)
        for k, v in zip(solved, part):
            out[k] = v
        return out

    def stopped_now():
        if gap is not None:
            now = state.gap_state()
            for name, values in zip(_GAP_INFO, now):
                info[name][solved] = values
            return now[1]
        now = state.stop_state()
        _many.spread_stop_state(info, solved, now)
        return now[1]

    try:
        if info is not None:
            if gap is not None:
                state.set_stop_gap(*gap)
            else:
                state.set_stop(*stop)
            if callback_func is not None:
                try:
                    callback_func.info = info
                except AttributeError:   # a bound method takes no attribute: wrap it in a function to read ``info``
                    pass
        xs = _cp_report_loop(state, costs, has_ineq, solved, best, all_x, spread, nb_max_iter, nb_iter_plot, callback_func, max_time, start,
                             None if info is None else stopped_now)
        if info is not None:
            stopped_now()
    finally:
        state.close()
    return xs, best, info


def chambolle_pock_ppd_many_until(problems, tol, check_every=10, x0=None, alpha=1, theta=1, nb_max_iter=10000, callback_func=None,
                                  max_time=None, nb_iter_plot=10):
    """``chambolle_pock_ppd_many`` with a stopping test per LP (extension; the reference has no stopping test): the list runs until
    every LP has stopped, at most ``nb_max_iter`` iterations.  Returns ``(xs, best_integer_solutions, info)``.

    The test is made inside the iteration kernel (``CPManyState.set_stop``), at the end of every iteration ``t`` of an LP with ``t %
    check_every == 0``, iterations counted from 1: the LP stops iff ``max(max|x_t - x_{t-1}|, max|y_t - y_{t-1}|) <= tol``, where
    ``x_t`` is the primal iterate and ``y_t`` the clamped dual iterate after ``t`` iterations; a NaN among the differences never
    stops.  A stopped LP keeps its iterate after ``t`` iterations, bit for bit that of ``chambolle_pock_ppd(...,
    nb_max_iter=t, order=ORDER_SEQUENTIAL)``, while the others go on.  ``tol`` is a finite float ``>= 0``, ``check_every`` an int
    ``>= 1``: a ``ValueError`` before the library is loaded otherwise, like every shape error.

    ``info`` is a dict of arrays over the whole list: ``iterations`` (int64: completed, for a stopped LP its stopping iteration),
    ``stopped`` (bool) and ``step`` (float64: the last evaluated step, ``+inf`` before the first test).  An LP without rows is
    stopped after 0 iterations with step 0.0.

    The cadence of reports is that of ``chambolle_pock_ppd_many``.  The loop ends at the first report index at which every LP is
    stopped (no callback for that index), at ``nb_max_iter``, or at ``max_time``.  In a callback a stopped LP's ``xs[k]`` is its
    final iterate, and its five numbers repeat the last row it had while it was running.  ``info`` is current at every callback:
    the same dict, updated in place, is set as the ATTRIBUTE ``callback_func.info`` before the first call (a function or any
    object that takes attributes; a bound method takes none and has to be wrapped in a function to read it).
    """
    stop = _many.check_stop(tol, check_every)
    return _cp_many_run(problems, x0, alpha, theta, nb_max_iter, callback_func, max_time, nb_iter_plot, stop)


def chambolle_pock_ppd_many_certified(problems, tol_gap, tol_feas, check_every=10, x0=None, alpha=1, theta=1, nb_max_iter=10000,
                                      callback_func=None, max_time=None, nb_iter_plot=10):
    """``chambolle_pock_ppd_many`` with a certificate as the stopping test per LP (extension; the reference evaluates the same
    lower bound, its ``energy2``, at its reports and stops on nothing): the list runs until every LP has stopped, at most
    ``nb_max_iter`` iterations.  Returns ``(xs, best_integer_solutions, info)``.

    The test is made inside the iteration kernel (``CPManyState.set_stop_gap``), at the end of every iteration ``t`` of an LP with
    ``t % check_every == 0``, iterations counted from 1, on the LP the solver holds (inequalities one-sided, ``y_t`` the clamped
    multipliers, dual feasible by construction): with ``primal = c.x_t``, ``lower_bound = sum_j min(d_j lb_j, d_j ub_j) - y_t.b``
    for ``d = c + K^T y_t`` and ``violation = max(max|A_eq x_t - b_eq|, max(A_ineq x_t - b_ineq), 0)`` the LP stops iff ``violation
    <= tol_feas`` and ``|primal - lower_bound| <= tol_gap * (1 + |primal| + |lower_bound|)`` with a finite left-hand side.  ``lower_bound`` is a bound on the
    LP's value whatever ``x_t`` is; it is ``-inf`` while a variable without a finite bound has ``d_j`` of the wrong sign, and such an
    LP, like one with a NaN, does not stop.  A stopped LP keeps its iterate after ``t`` iterations, bit for bit that of
    ``chambolle_pock_ppd(..., nb_max_iter=t, order=ORDER_SEQUENTIAL)``, while the others go on.  ``tol_gap`` and ``tol_feas`` are
    finite floats ``>= 0``, ``check_every`` an int ``>= 1``: a ``ValueError`` before the library is loaded otherwise, like every shape
    error.

    ``info`` is a dict of arrays over the whole list: ``iterations`` (int64: completed, for a stopped LP its stopping iteration),
    ``stopped`` (bool), and ``primal``, ``lower_bound``, ``violation`` (float64: the last evaluated certificate; ``+inf``, ``-inf``,
    ``+inf`` before the first).  The two sums are in the kernel's own fixed order.  An LP without rows is stopped after 0
    iterations; its ``primal`` and ``lower_bound`` are both the cost of its box vertex and its ``violation`` is 0.

    Reports, callbacks, ``callback_func.info`` and the end of the loop are those of ``chambolle_pock_ppd_many_until``.
    """
    tol_gap, every = _many.check_stop(tol_gap, check_every, "tol_gap")
    tol_feas, _ = _many.check_stop(tol_feas, check_every, "tol_feas")
    return _cp_many_run(problems, x0, alpha, theta, nb_max_iter, callback_func, max_time, nb_iter_plot, None, (tol_gap, tol_feas, every))
