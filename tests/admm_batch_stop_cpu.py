"""numpy restatement of the per-instance stopping rule of the batched ADMM solver (csrc/slp_admm_batch.hip,
``ADMMBatchState.set_stop``), on top of tests/admm_stop_cpu.py: the rule per instance is the list solver's, the semantics are the
batch's.

Per instance ``k`` the curves ``(residual_t, step_t)``, ``t = 1 .. T``, are ``admm_stop_cpu.oracle_curves`` on the instance alone
(``test_gpu_admm_batch._of_instance``).  The batch has ONE iteration counter ``t``, counted from 1 over the life of the state,
armed or not, and a stopped instance stays stopped for the life of the state.  A run is a ``schedule``: a list of
``(after, tol_residual, tol_step, check_every)`` with increasing ``after`` -- a ``set_stop`` call made when ``after`` iterations
are complete; ``tol_residual=None`` turns the test off -- and the ``total`` iterations asked of the state.  Within a segment an
instance that still runs follows ``admm_stop_cpu.stop_state``; across segments its flag is kept and so are the last evaluated
residual and step (``+inf`` before the first test).
"""
import numpy as np

import admm_stop_cpu


def instance_curves(args, k, nb_iter, of_instance):
    """``(residual, step)`` of instance ``k`` of the batch ``args`` for ``t = 1 .. nb_iter``; ``of_instance``:
    ``test_gpu_admm_batch._of_instance``."""
    problem, x0 = of_instance(args, k)
    return admm_stop_cpu.oracle_curves(problem, nb_iter, x0=x0)


def batch_curves(args, nb_iter, of_instance):
    """The curves of every instance of the batch, a tuple of read-only ``(residual, step)`` pairs."""
    out = []
    for k in range(args["cs"].shape[0]):
        curves = instance_curves(args, k, nb_iter, of_instance)
        for c in curves:
            c.setflags(write=False)
        out.append(curves)
    return tuple(out)


def instance_state(residual, step, schedule, total):
    """``(iterations, stopped, residual, step)`` of one instance after ``total`` iterations of a state armed by ``schedule``."""
    state = (0, False, np.inf, np.inf)
    for i, (after, tol_residual, tol_step, check_every) in enumerate(schedule):
        end = min(total, schedule[i + 1][0]) if i + 1 < len(schedule) else total
        assert i == 0 or after > schedule[i - 1][0]
        if end <= after:
            break
        if tol_residual is None:   # off: the instance goes on untested
            state = (end, False, state[2], state[3])
            continue
        state = admm_stop_cpu.stop_state(residual, step, tol_residual, tol_step, check_every, end, after=after, before=state[2:])
        if state[1]:
            return state           # sticky: later segments do not look at it again
    return (total,) + tuple(state[1:])


def stop_state(curves, schedule, total):
    """``(iterations, stopped, residual, step)`` as ``ADMMBatchState.stop_state`` reports them, arrays over the batch (int64, bool,
    float64, float64).  ``schedule``: the list described above, or one ``(tol_residual, tol_step, check_every)`` armed before the
    first iteration."""
    if len(schedule) == 3 and not isinstance(schedule[0], (tuple, list)):
        schedule = [(0,) + tuple(schedule)]
    rows = [instance_state(r, s, schedule, total) for r, s in curves]
    return (np.array([r[0] for r in rows], dtype=np.int64), np.array([r[1] for r in rows], dtype=bool),
            np.array([r[2] for r in rows], dtype=np.float64), np.array([r[3] for r in rows], dtype=np.float64))


def stopping_iterations(curves, tol_residual, tol_step, check_every, total):
    """Per instance its stopping iteration within ``total`` iterations of a state armed before the first one, or ``None``."""
    return [admm_stop_cpu.stopping_iteration(r[:total], s[:total], tol_residual, tol_step, check_every) for r, s in curves]
