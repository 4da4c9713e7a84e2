"""The cases of the bound cut-off of dual gradient ascent on a list (``DeviceDGAMany.set_cutoff``, csrc/slp_dga_many.hip), shared by
tests/test_dga_many_bound_host.py (no GPU: the cases are what the GPU test relies on) and tests/test_gpu_dga_many_bound.py.

The fifteen small LPs of tests/test_dga_many_stop_host.py over 130 iterations, their step curves and their bound curves --
``dga_cpu.device_energy`` on the ``dga_cpu`` states, which shares no text with the device -- and one vector of cut-offs chosen so
that every way of stopping occurs at every cadence the GPU test uses.  Computed once per process; do not modify."""
import functools

import numpy as np
import scipy.sparse

import dga_batch_stop_cpu
from dga_cpu import device_energy, dual_argmin, dual_energy
from test_dga_many_stop_host import ITERATIONS, fifteen, fifteen_states

TOL = 1e-4               # LPs 2, 4 and 10 never meet it in 130 iterations, at any cadence
EVERY = (1, 4, 10)
INF = np.inf
# list index -> (kind, check): the cut-off is the LP's own restated bound at that check (a multiple of 20: a check at every cadence)
EQUAL = {0: 40, 3: 40, 6: 60, 7: 20, 10: 20}   # met by equality, if not before
ABOVE = {11: 20, 12: 40}                       # np.nextafter upwards of it: reached there and not met
NEVER = {4: 1e6}                               # finite and out of reach: the bound is recorded at every check, the LP runs on
BOTH = 3                                       # stops at 40 on its step at every cadence, and its cut-off is its bound at 40


@functools.lru_cache(maxsize=None)
def fifteen_curves():
    """Per LP ``(steps, bounds)`` over ``t = 1 .. ITERATIONS``; shared, read-only."""
    out = []
    for args, states in zip(fifteen(), fifteen_states()):
        steps, bounds = dga_batch_stop_cpu.curves_of(states, lambda y_eq, y_ineq, a=args: device_energy(*a, y_eq, y_ineq))
        steps.setflags(write=False)
        bounds.setflags(write=False)
        out.append((steps, bounds))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _targets():
    bounds = [b for _, b in fifteen_curves()]
    t = np.full(15, INF)
    for k, check in EQUAL.items():
        t[k] = bounds[k][check - 1]
    for k, check in ABOVE.items():
        t[k] = np.nextafter(bounds[k][check - 1], INF)
    for k, value in NEVER.items():
        t[k] = value
    t.setflags(write=False)
    return t


def targets():
    """The fifteen cut-offs (``+inf``: none); read-only."""
    return _targets()


def expected(rules, total=ITERATIONS):
    """``(iterations, stopped, step, bound, reason)`` of the restatement for the fifteen LPs under ``rules``, a list of ``(after,
    tol, targets, check_every)`` (tests/dga_batch_stop_cpu.py)."""
    curves = fifteen_curves()
    return dga_batch_stop_cpu.stop_state([s for s, _ in curves], [b for _, b in curves], rules, total)


SCHEDULE_TOTAL = 60


@functools.lru_cache(maxsize=None)
def schedule():
    """The rules of a state whose test is armed late, changed, reduced to the step and turned off, ``(after, tol, targets,
    check_every)``: cut-offs from 7 iterations on; at 26 other cut-offs and the cadence 10 -> 4 (LP 2's is its bound at 36, the last
    check of that rule; LPs 0 and 6 get theirs at 28 and 32; LP 12 loses its own); at 36 the tolerance alone; off at 50."""
    bounds = [b for _, b in fifteen_curves()]
    second = np.array(targets())
    second[0], second[6], second[2], second[12] = bounds[0][27], bounds[6][31], bounds[2][35], INF
    second.setflags(write=False)
    return ((7, TOL, targets(), 10), (26, TOL, second, 4), (36, TOL, None, 4), (50, None, None, 1))


def bound_slack(args, y_eq, y_ineq):
    """The rounding of a dual energy summed in any order, as ``DgaLP.bound_slack`` of tools/fuzz_batched.py states it:
    ``gamma_(n + m + 2) (sum |c_bar_j| max(|lb_j|, |ub_j|) + sum |y_i b_i|)``."""
    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = args
    c_bar, _ = dual_argmin(c, a_eq, a_ineq, lb, ub, y_eq, y_ineq)
    m = (0 if a_eq is None else a_eq.shape[0]) + (0 if a_ineq is None else a_ineq.shape[0])
    k = c.size + m + 2
    gamma = k * 2.0 ** -53 / (1 - k * 2.0 ** -53)
    terms = np.sum(np.abs(c_bar) * np.maximum(np.abs(lb), np.abs(ub)))
    if a_eq is not None:
        terms += np.sum(np.abs(y_eq * b_eq))
    if a_ineq is not None:
        terms += np.sum(np.abs(y_ineq * b_upper))
    return gamma * terms


def energies_agree(args, y_eq, y_ineq):
    """``device_energy`` lies within ``bound_slack`` of ``dual_energy``, the same sums in numpy's order."""
    e, d = dual_energy(*args, y_eq, y_ineq), device_energy(*args, y_eq, y_ineq)
    return abs(e - d) <= bound_slack(args, y_eq, y_ineq)


def integer_lp(n, m, m_eq=0, seed=0):
    """The construction of ``integer_lp`` (tests/test_gpu_dga.py) for a given shape: ``m`` rows of at most 4 integer entries, one per
    column stratum, the first ``m_eq`` of them equalities met by an integer point inside integer bounds, integer costs and slacks."""
    rng = np.random.RandomState(1000 * seed + 7 * n + m)
    k = min(n, 4)
    cols = (np.arange(k) * (n // k) + rng.randint(0, n // k, size=(m, k))).astype(np.int32)
    vals = np.round(10 * rng.randn(m, k))
    vals[vals == 0] = 1.0
    a = scipy.sparse.csr_matrix((vals.ravel(), cols.ravel(), np.arange(0, m * k + 1, k)), shape=(m, n))
    lb = rng.randint(-5, 1, size=n).astype(np.float64)
    ub = lb + rng.randint(1, 10, size=n)
    xf = lb + np.floor(rng.rand(n) * (ub - lb + 1))
    ax = a @ xf
    b = ax + rng.randint(0, 50, size=m)
    b[:m_eq] = ax[:m_eq]
    c = np.round(10 * rng.randn(n))
    return c, a[:m_eq].tocsr(), b[:m_eq], (a[m_eq:].tocsr() if m_eq < m else None), (b[m_eq:] if m_eq < m else None), lb, ub
