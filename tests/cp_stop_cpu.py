"""numpy restatement of the per-LP stopping rule of the Chambolle-Pock list solver (csrc/slp_cp_many.hip, ``CPManyState.set_stop``).

Iterations count from 1.  With ``x_t`` the primal iterate and ``y_t = [y_eq; y_ineq]`` the clamped dual iterate after ``t``
iterations, ``step_t = max(np.max|x_t - x_{t-1}|, np.max|y_t - y_{t-1}|)`` (a NaN stays, as ``np.max`` keeps it), and an LP stops at
the first ``t`` with ``t % check_every == 0`` and ``step_t <= tol``.  The maxima are exact in any order, so the device's decision
must be this one bit for bit.

The iterates come from ``oracle.chambolle_pock_ppd(..., iterate_hook=...)``: call ``i`` of the hook (``niter = i``) sees ``x_{i+1}``
(after the primal half of iteration ``i + 1``) and ``y_i`` (before its dual half), so ``T + 1`` iterations of the oracle give
``x_1 .. x_T`` and ``y_0 .. y_T``.  The oracle raises at its first report for an LP without inequality rows, as the reference
does: for such an LP the iterates have to come from elsewhere (``steps_of`` takes any).
"""
import numpy as np


def oracle_iterates(problem, nb_iter, x0=None):
    """``([x_0 .. x_T], [y_0 .. y_T])`` of the 8-tuple ``problem`` for ``T = nb_iter``, from the oracle."""
    from oracle import oracle

    n = np.asarray(problem[0]).size
    xs, ys = [np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)], []

    def hook(niter, x, y_eq, y_ineq):
        xs.append(np.array(x, copy=True))
        ys.append(np.concatenate([np.array(v, copy=True) for v in (y_eq, y_ineq) if v is not None]))

    oracle.chambolle_pock_ppd(*problem, x0=x0, nb_max_iter=nb_iter + 1, nb_iter_plot=10 ** 9, iterate_hook=hook)
    assert len(ys) == nb_iter + 1
    return xs[:nb_iter + 1], ys


def steps_of(xs, ys):
    """``step_t`` for ``t = 1 .. T`` from ``[x_0 .. x_T]`` and ``[y_0 .. y_T]``; entry ``t - 1`` belongs to iteration ``t``."""
    assert len(xs) == len(ys)
    with np.errstate(invalid="ignore"):
        return np.array([max(_max_abs(xs[t] - xs[t - 1]), _max_abs(ys[t] - ys[t - 1]), key=_nan_first)
                         for t in range(1, len(xs))], dtype=np.float64)


def _max_abs(v):
    """``np.max|v|``, 0.0 for no entry (as ``admm_stop_cpu._max_abs``: a dual block whose only row was dropped); a NaN stays."""
    return float(np.max(np.abs(v))) if v.size else 0.0


def _nan_first(v):
    """Orders a NaN above everything: ``max(a, b, key=_nan_first)`` is ``np.max([a, b])``."""
    return (1, 0.0) if v != v else (0, v)


def stopping_iteration(steps, tol, check_every, after=0):
    """The first iteration ``t > after`` with ``t % check_every == 0`` and ``step_t <= tol``, or ``None`` within ``len(steps)``."""
    for t in range(after + 1, len(steps) + 1):
        if t % check_every == 0 and steps[t - 1] <= tol:
            return t
    return None


def stop_state(steps, tol, check_every, total, after=0, step_before=np.inf):
    """``(iterations, stopped, step)`` as ``CPManyState.stop_state`` reports them for one LP after a run that was armed at
    iteration ``after`` (the last evaluated step then ``step_before``) and asked for ``total`` iterations of its life."""
    t = stopping_iteration(steps[:total], tol, check_every, after)
    if t is not None:
        return t, True, steps[t - 1]
    last = total - total % check_every   # the last check iteration
    return total, False, (steps[last - 1] if last > after else step_before)
