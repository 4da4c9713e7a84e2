"""numpy restatement of the per-LP stopping rule of the ADMM list solver (csrc/slp_admm_many.hip, ``ADMMManyState.set_stop``).

Iterations count from 1; iteration ``t`` is the right-hand side, the sweep that gives ``x_t`` (all ``N = n + m_ineq`` columns of the
standard form) and the multiplier update that gives ``lambda_t``.  With ``a``, ``b`` the standard form of ``oracle.admm_setup``,

    residual_t = np.max|a x_t - b|          (0.0 for an LP without rows)
    step_t     = np.max|x_t - x_{t-1}|      (x_0 the stored start, ``admm_setup``'s ``x0``)

(a NaN stays, as ``np.max`` keeps it), and an LP stops at the first ``t`` with ``t % check_every == 0``, ``residual_t <=
tol_residual`` and ``step_t <= tol_step``.  The maxima are exact in any order and ``a x_t - b`` is the value the multiplier update
forms, so the device's decision must be this one bit for bit.

The iterates come from ``oracle.lp_admm(..., iterate_hook=...)``: call ``i`` of the hook sees ``x_{i+1}`` over all ``N``, so ``nb_iter =
T - 1`` gives ``x_1 .. x_T``; ``curves_of`` takes the iterates of any source.
"""
import numpy as np


def _max_abs(v):
    """``np.max|v|``, 0.0 for no entry; a NaN stays."""
    return float(np.max(np.abs(v))) if v.size else 0.0


def residual_of(a, b, x):
    """``np.max|a x - b|`` with the oracle's product: one accumulator per row, storage order."""
    from oracle import oracle

    with np.errstate(invalid="ignore"):
        return _max_abs(oracle.matvec(a, x) - b) if a.shape[0] else 0.0


def curves_of(xs, residuals):
    """``(residual, step)``, two arrays over ``t = 1 .. T`` (entry ``t - 1`` belongs to iteration ``t``), from the iterates ``[x_0 ..
    x_T]`` over all ``N`` columns and the residuals ``[residual_1 .. residual_T]``."""
    assert len(xs) == len(residuals) + 1
    with np.errstate(invalid="ignore"):
        step = np.array([_max_abs(xs[t] - xs[t - 1]) for t in range(1, len(xs))], dtype=np.float64)
    return np.array(residuals, dtype=np.float64), step


def oracle_curves(problem, nb_iter, x0=None, **kw):
    """``(residual, step)`` of the 8-tuple ``problem`` for ``t = 1 .. nb_iter``, from the oracle."""
    from oracle import oracle

    s = oracle.admm_setup(*problem, x0, **kw)
    a, b = s["a"], s["b"]
    xs, residuals = [np.array(s["x0"], dtype=np.float64, copy=True)], []

    def hook(i, x, x_full, lam):
        xs.append(np.array(x_full, dtype=np.float64, copy=True))
        residuals.append(residual_of(a, b, xs[-1]))

    oracle.lp_admm(*problem, x0=x0, nb_iter=nb_iter - 1, nb_iter_plot=10 ** 9, iterate_hook=hook, **kw)
    assert len(residuals) == nb_iter
    return curves_of(xs, residuals)


def stopping_iteration(residual, step, tol_residual, tol_step, check_every, after=0):
    """The first iteration ``t > after`` with ``t % check_every == 0``, ``residual_t <= tol_residual`` and ``step_t <= tol_step``, or
    ``None`` within ``len(step)``."""
    assert len(residual) == len(step)
    for t in range(after + 1, len(step) + 1):
        if t % check_every == 0 and residual[t - 1] <= tol_residual and step[t - 1] <= tol_step:
            return t
    return None


def stop_state(residual, step, tol_residual, tol_step, check_every, total, after=0, before=(np.inf, np.inf)):
    """``(iterations, stopped, residual, step)`` as ``ADMMManyState.stop_state`` reports them for one LP after a run that was armed
    at iteration ``after`` (the last evaluated residual and step then ``before``) and asked for ``total`` iterations of its life."""
    t = stopping_iteration(residual[:total], step[:total], tol_residual, tol_step, check_every, after)
    if t is not None:
        return t, True, residual[t - 1], step[t - 1]
    last = total - total % check_every   # the last check iteration
    if last > after:
        return total, False, residual[last - 1], step[last - 1]
    return total, False, before[0], before[1]
