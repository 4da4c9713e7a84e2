"""numpy restatement of the per-instance stopping rule of the batched dual gradient ascent (csrc/slp_dga_batch.hip,
``DeviceDGABatch.set_stop``), on a step curve and a bound curve per instance.

Iterations ``t`` count from 1 over the life of the state, the same number for every instance; entry ``t - 1`` of a curve belongs
to iteration ``t``: ``steps[k][t - 1] = max|y_t - y_{t-1}|`` of instance ``k`` (``dga_stop_cpu.steps_of``: after the clamp, 0 from a
kind of rows that does not move, a NaN stays) and ``bounds[k][t - 1]`` the dual energy of ``y_t``.  A rule ``(after, tol, targets,
check_every)`` is armed when ``after`` iterations are complete and holds until the next one: ``tol`` None = no step test,
``targets`` None = no bound test (else one cut-off per instance, ``+inf`` = none for that instance), both None = the test is off.
At the end of an iteration ``t > after`` with ``t % check_every == 0`` an instance that is neither frozen nor stopped stops iff
``steps[k][t - 1] <= tol`` or ``bounds[k][t - 1] >= targets[k]``; both are looked at, so the reason (bit 0 step, bit 1 bound) may
name both.  A NaN in either quantity meets nothing, and from the iteration at which an instance's status carries the NaN bit
(``nan_from[k]``) it meets nothing at all.  A stopped instance stays stopped under every later rule.  The step is recorded at every
check, the bound at the checks of a rule with cut-offs; before the first they are ``+inf`` and ``-inf``.

The search for the first check that meets a tolerance is ``dga_stop_cpu.stopping_iteration`` -- for the bound on the negated curve,
``-bound <= -target`` being ``bound >= target`` for every pair of floats, infinities included, and false for a NaN."""
import numpy as np

from dga_stop_cpu import steps_of, stopping_iteration


def curves_of(states, energy):
    """``(steps, bounds)`` over ``t = 1 .. T`` of one instance from ``dga_cpu``'s states with keys ``-1 .. T - 1``; ``energy(y_eq,
    y_ineq)`` gives the dual energy of a pair of multipliers."""
    total = len(states) - 1
    return steps_of(states), np.array([energy(states[t - 1][1], states[t - 1][2]) for t in range(1, total + 1)])


def stop_state(steps, bounds, rules, total, frozen=None, nan_from=None):
    """``(iterations, stopped, step, bound, reason)`` as ``DeviceDGABatch.stop_state`` reports them after ``total`` iterations of
    the state's life under ``rules``, a list of ``(after, tol, targets, check_every)`` with increasing ``after``."""
    batch = len(steps)
    frozen = np.zeros(batch, dtype=bool) if frozen is None else np.asarray(frozen, dtype=bool)
    nan_from = [None] * batch if nan_from is None else nan_from
    iterations, reason = np.full(batch, total, dtype=np.int64), np.zeros(batch, dtype=np.int32)
    step, bound = np.full(batch, np.inf), np.full(batch, -np.inf)
    assert [r[0] for r in rules] == sorted(r[0] for r in rules)
    for k in range(batch):
        if frozen[k]:
            iterations[k] = 0
            continue
        # what the decision sees: nothing from the iteration on at which the NaN bit is up
        ds, db = np.array(steps[k], dtype=np.float64), np.array(bounds[k], dtype=np.float64)
        if nan_from[k] is not None:
            ds[nan_from[k] - 1:] = np.nan
            db[nan_from[k] - 1:] = np.nan
        for i, (after, tol, targets, every) in enumerate(rules):
            until = min(rules[i + 1][0] if i + 1 < len(rules) else total, total)
            if after >= until or (tol is None and targets is None):
                continue
            target = None if targets is None else float(np.broadcast_to(targets, (batch,))[k])
            found = []
            if tol is not None:
                found.append(stopping_iteration(ds[:until], tol, every, after))
            if target is not None and target < np.inf:
                found.append(stopping_iteration(-db[:until], -target, every, after))
            found = [t for t in found if t is not None]
            last = min(found) if found else until - until % every   # the stopping check, else the last check of the rule
            if last > after:
                step[k] = steps[k][last - 1]
                if targets is not None:
                    bound[k] = bounds[k][last - 1]
            if found:
                iterations[k] = last
                by_step = tol is not None and ds[last - 1] <= tol
                by_bound = target is not None and target < np.inf and db[last - 1] >= target
                reason[k] = (1 if by_step else 0) | (2 if by_bound else 0)
                break
    return iterations, reason != 0, step, bound, reason
