"""numpy restatement of the per-LP stopping rule of dual gradient ascent on a list (csrc/slp_dga_many.hip,
``DeviceDGAMany.set_stop``), on the states of tests/dga_cpu.py.

Iterations count from 1.  With ``y_t = [y_eq; y_ineq]`` the multipliers after ``t`` iterations (the inequality part after its
clamp, ``y_0`` the start), ``step_t = np.max|y_t - y_{t-1}|`` over all rows (a NaN stays, as ``np.max`` keeps it); a kind of rows
that does not move in iteration ``t`` contributes 0 -- its multipliers are then the same array, whatever it holds.  An LP stops at
the first ``t`` with ``t % check_every == 0`` and ``step_t <= tol``.  The maximum is exact in any order, so the device's decision
must be this one bit for bit wherever its iterates are ``dga_cpu``'s.

``dga_cpu`` numbers its iterations from 0 and keeps, under key ``it``, the state after ``it + 1`` iterations (the x of the top of
iteration ``it``: what the reference returns after ``it + 1``); key -1 is the start.  So ``y_t`` is ``states[t - 1]``.
"""
import numpy as np

from dga_cpu import dga_cpu


def states_of(args, nb_iter, order="reference"):
    """``{it: (x, y_eq, y_ineq, draws)}`` for ``it = -1 .. nb_iter - 1`` of the LP ``args`` as ``dga_cpu`` takes it."""
    return dga_cpu(*args, nb_max_iter=nb_iter, order=order, keep=range(nb_iter))


def _kind_step(new, old):
    """``np.max|new - old|`` of one kind of rows; 0.0 for a kind that is absent or did not move."""
    if new is None or new.size == 0 or np.array_equal(new, old, equal_nan=True):
        return 0.0
    with np.errstate(invalid="ignore"):
        return float(np.max(np.abs(new - old)))


def steps_of(states):
    """``step_t`` for ``t = 1 .. T`` from ``dga_cpu``'s states with keys ``-1 .. T - 1``; entry ``t - 1`` belongs to iteration
    ``t``.  A dual-infeasible start (key -1 only) has no iteration: an empty array."""
    total = len(states) - 1
    assert sorted(states) == list(range(-1, total))
    out = np.zeros(total)
    for t in range(1, total + 1):
        (_, e1, i1, _), (_, e0, i0, _) = states[t - 1], states[t - 2]
        a, b = _kind_step(e1, e0), _kind_step(i1, i0)
        out[t - 1] = np.nan if (a != a or b != b) else max(a, b)
    return out


def stopping_iteration(steps, tol, check_every, after=0):
    """The first iteration ``t > after`` with ``t % check_every == 0`` and ``step_t <= tol``, or ``None`` within ``len(steps)``."""
    for t in range(after + 1, len(steps) + 1):
        if t % check_every == 0 and steps[t - 1] <= tol:
            return t
    return None


def stop_state(steps, tol, check_every, total, after=0, step_before=np.inf):
    """``(iterations, stopped, step)`` as ``DeviceDGAMany.stop_state`` reports them for one LP after a run that was armed at
    iteration ``after`` (the last evaluated step then ``step_before``) and asked for ``total`` iterations of its life."""
    t = stopping_iteration(steps[:total], tol, check_every, after)
    if t is not None:
        return t, True, steps[t - 1]
    last = total - total % check_every   # the last check iteration
    return total, False, (steps[last - 1] if last > after else step_before)
