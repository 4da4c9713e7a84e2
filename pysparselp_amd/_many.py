"""What the list forms of the solvers (LPs with matrices of their own, one workgroup per LP: ``chambolle_pock_ppd_many``,
``lp_admm_many``, ``dual_gradient_ascent_many``) share on the host: the checks of one LP of the list, the stacking of the LPs'
matrices and the common part of the device states.  Private; numpy only, and nothing here loads the library -- every refusal
below is a ``ValueError`` raised before a caller touches the GPU.  What the batched forms use too is in ``_batch.py``."""
import numbers

import numpy as np

from . import _lib
from ._batch import concat, split_by

_TUPLE = "(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub)"


def count_problems(problems):
    """The length of ``problems``, a non-empty sequence of 8-tuples."""
    try:
        count = len(problems)
    except TypeError:
        raise ValueError(f"problems must be a sequence of 8-tuples {_TUPLE}") from None
    if count < 1:
        raise ValueError("an empty list of LPs: problems needs at least one entry")
    return count


def unpack_problem(k, problem):
    """The 8 entries of LP ``k``."""
    try:
        count = len(problem)
    except TypeError:
        count = -1
    if count != 8:
        raise ValueError(f"LP {k} is not a tuple of 8 entries {_TUPLE}")
    return tuple(problem)


def check_cost(k, name, c, finite=False):
    """The cost vector of LP ``k`` as a contiguous float64 array of shape ``(n,)`` with ``n >= 1``."""
    c = _lib.f64(c)
    if c.ndim != 1 or c.size < 1:
        raise ValueError(f"LP {k}: {name} has shape {c.shape}, expected (n,) with n >= 1")
    return check_vector(k, name, c, c.shape, "", finite=finite)


def check_vector(k, name, v, shape, against, finite=False, no_nan=False):
    """``v`` of LP ``k`` as a contiguous float64 array of the given shape; ``against`` says in the refusal where the shape comes
    from, e.g. ``"c has 5 entries"``."""
    v = _lib.f64(v)
    if v.shape != shape:
        raise ValueError(f"LP {k}: {name} has shape {v.shape}, {against}")
    if finite and not np.all(np.isfinite(v)):
        raise ValueError(f"LP {k}: {name} has an entry that is not finite")
    if no_nan and np.any(np.isnan(v)):
        raise ValueError(f"LP {k}: {name} has a NaN")
    return v


def check_csr(k, name, a, n, against):
    """``a`` (``indptr``, ``indices``, ``data``, ``shape``) of LP ``k`` is a well-formed CSR matrix over ``n`` columns."""
    if a.shape[1] != n:
        raise ValueError(f"LP {k}: {name} has {a.shape[1]} columns, {against}")
    if a.indptr.shape != (a.shape[0] + 1,) or a.indptr[0] != 0 or np.any(np.diff(a.indptr) < 0) or a.indptr[-1] != a.indices.size \
            or a.indices.size != a.data.size:
        raise ValueError(f"LP {k}: {name} is not a well-formed CSR matrix")
    if a.indices.size and (a.indices.min() < 0 or a.indices.max() >= n):
        raise ValueError(f"LP {k}: {name} has a column index outside [0, {n})")


def check_starts(x0, lps, finite=False):
    """``x0`` checked against the validated LPs (``lps[k][0]`` is the cost vector): ``None``, or a list with one float64 start (or
    ``None``) per LP."""
    if x0 is None:
        return None
    try:
        given = len(x0)
    except TypeError:
        given = -1
    if given != len(lps):
        raise ValueError(f"x0 must be None or a sequence of {len(lps)} starts, one per LP")
    return [None if v is None else check_vector(k, "x0", v, lps[k][0].shape, f"c has {lps[k][0].size} entries", finite=finite)
            for k, v in enumerate(x0)]


def concat_starts(x0, n):
    """The starts of ``check_starts`` as one contiguous array over all LPs (zeros where an LP has none), or ``None`` when no LP
    has one; ``n``: the number of variables per LP."""
    if x0 is None or all(v is None for v in x0):
        return None
    return _lib.f64(np.concatenate([np.zeros(int(nk)) if v is None else _lib.f64(v) for v, nk in zip(x0, n)]))


def stack_blocks(blocks, col_offsets=None):
    """The CSR blocks ``(indptr, indices, data)`` stacked by rows: ``(indptr int64, indices int32, data float64)`` with every row
    in its own storage order; the column indices of block ``k`` are shifted by ``col_offsets[k]`` when offsets are given."""
    ptr, idx, val, entries = [np.zeros(1, dtype=np.int64)], [], [], 0
    for k, (p, j, v) in enumerate(blocks):
        ptr.append(entries + np.asarray(p[1:], dtype=np.int64))
        idx.append(j if col_offsets is None else np.asarray(j, dtype=np.int64) + col_offsets[k])
        val.append(v)
        entries += int(p[-1])
    return concat(ptr, np.int64), concat(idx, np.int32), concat(val, np.float64)


def check_stop(tol, check_every, name="tol"):
    """The tolerance and the cadence of a per-LP stopping test as ``(float, int)``: ``tol`` a finite number ``>= 0``,
    ``check_every`` an int ``>= 1`` (iterations between two tests).  ``name``: what a refusal calls the tolerance, for a test that
    has more than one."""
    if isinstance(tol, bool) or not isinstance(tol, numbers.Real) or not np.isfinite(tol) or tol < 0:
        raise ValueError(f"{name} must be a finite float >= 0, not {tol!r}")
    if isinstance(check_every, bool) or not isinstance(check_every, numbers.Integral) or check_every < 1:
        raise ValueError(f"check_every must be an int >= 1, not {check_every!r}")
    return float(tol), int(check_every)


def new_stop_info(count, solved, residual=False):
    """The stop state of a whole list before its first iteration, a dict of arrays over the ``count`` LPs: ``iterations`` (int64),
    ``stopped`` (bool), ``step`` (float64, the last evaluated step) and, with ``residual`` (a test on two quantities), ``residual``
    (float64, the last evaluated residual).  The LPs outside ``solved`` take no part in the iterations: they are stopped after 0
    iterations with step (and residual) 0.0; the others run, their step ``+inf`` until the first test."""
    info = dict(iterations=np.zeros(count, dtype=np.int64), stopped=np.ones(count, dtype=bool), step=np.zeros(count))
    if residual:
        info["residual"] = np.zeros(count)
    info["stopped"][solved] = False
    for name in ("step", "residual")[:2 if residual else 1]:
        info[name][solved] = np.inf
    return info


def spread_stop_state(info, solved, state):
    """``state`` -- ``(iterations, stopped, step)`` of the LPs ``solved``, as a device state's ``stop_state()`` returns them, or
    ``(iterations, stopped, residual, step)`` of a state that tests two quantities -- written into ``info`` (``new_stop_info``) in
    place: whoever holds the dict sees the current values."""
    names = ("iterations", "stopped", "step") if len(state) == 3 else ("iterations", "stopped", "residual", "step")
    for name, values in zip(names, state):
        info[name][solved] = values


class ManyState:
    """What the device states of a list share.  A subclass sets ``_PREFIX`` (its C entry points are ``<_PREFIX>_destroy``,
    ``<_PREFIX>_form``, ``<_PREFIX>_get_*``), ``_LIVE`` (``<_LIVE>_set_compaction``, ``<_LIVE>_live_state``), ``count``, the loaded
    library ``_l`` and its handle ``_h``."""

    FORMS = ("lds", "global")
    _PREFIX = None
    _LIVE = None

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._l, self._PREFIX + "_destroy")(self._h)
            self._h = None

    __del__ = close

    def _of_lp(self, k):
        if not 0 <= int(k) < self.count:
            raise IndexError(f"LP {k} of {self.count}")
        return int(k)

    def form(self, k):
        """``"lds"`` or ``"global"``: where LP ``k`` keeps its iterates during a launch."""
        return self.FORMS[int(getattr(self._l, self._PREFIX + "_form")(self._h, self._of_lp(k)))]

    def set_compaction(self, on=True):
        """Turns compaction on or off (``<_LIVE>_set_compaction``, include/slp_hip_ext_many_live.h; off after the constructor).
        While it is on, a call on an armed state (``iterate`` and the two half steps) first reads the per-LP records back -- one
        download, which synchronises -- and every launch of a form then runs over a list of that form's LPs not yet stopped, which
        the device builds in front of it: the grid is the number of LPs of the form live when the call began, the iterations one
        launch holds are those of that many workgroups, and a form without a live LP launches nothing.  An unarmed state has no
        stopped LP and launches as without compaction.  Every LP's iterates, record and report are bit for bit those of the state
        without it."""
        if not isinstance(on, (bool, int, np.integer)) or int(on) not in (0, 1):
            raise ValueError(f"on must be True or False, not {on!r}")
        _lib.check(getattr(self._l, self._LIVE + "_set_compaction")(self._h, int(on)))

    def live_state(self):
        """``(live, order, launched, cap)`` (``<_LIVE>_live_state``): ``live`` the numbers of live LPs of the two forms (lds,
        global; an int64 array of length 2), ``order`` the live LPs as the device lists them (int32: those of the lds form in
        increasing order, then those of the global form in increasing order), ``launched`` the workgroups of each form's last
        iteration launch and ``cap`` the iterations per launch each form was held to in the last call that launched it (int64
        arrays of length 2, 0 before the first launch).  Works with compaction on or off; reading it synchronises."""
        live, launched, cap = (np.zeros(2, dtype=np.int64) for _ in range(3))
        order = np.zeros(self.count, dtype=np.int32)
        _lib.check(getattr(self._l, self._LIVE + "_live_state")(self._h, _lib.ptr(live), _lib.ptr(order), _lib.ptr(launched), _lib.ptr(cap)))
        assert np.all(order[int(live.sum()):] == -1)
        return live, order[:int(live.sum())].copy(), launched, cap

    def _per_lp(self, what, sizes, *args):
        """The flat vector ``<_PREFIX>_get_<what>`` writes, cut into one array per LP."""
        out = np.empty(int(sizes.sum()))
        _lib.check(getattr(self._l, f"{self._PREFIX}_get_{what}")(self._h, _lib.ptr(out), *args))
        return split_by(out, sizes)
