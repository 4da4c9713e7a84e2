"""The batches the batched dual gradient ascent is tested on (tests/test_dga_batch_host.py without a GPU,
tests/test_gpu_dga_batch.py on one): four fixture LPs, six cost vectors each, and their iterates by tests/dga_cpu.py with
``order="reference"`` -- the restatement tests/test_dga_host.py pins to the reference bit for bit.  Computed once per process."""
import numpy as np

from conftest import load_golden
from dga_cpu import dga_cpu
from test_dga_host import dga_args

BATCH_CASES = ("potts8", "random0", "random1", "sc50a")
STOPS = (0, 1, 10, 50, 100)   # iterations (0-based) at which the states are compared: after 1, 2, 11, 51, 101 iterations
_CACHE = {}


def six_costs(c):
    """The fixture's cost, a multiple, its reversal, a perturbation, its negative and an unrelated one."""
    rs = np.random.RandomState(7)
    n = c.size
    return np.array([c, 2.0 * c, c[::-1].copy(), c * (1 + 0.25 * rs.rand(n)), -c, np.round(8 * rs.randn(n)) / 8])


def batch_case(case):
    """``(args, costs)``: the fixture's ``(c, a_eq, b_eq, a_ineq, b_upper, lb, ub)`` and its six costs."""
    if ("case", case) not in _CACHE:
        args = dga_args(load_golden("lp_" + case))
        _CACHE["case", case] = (args, six_costs(args[0]))
    return _CACHE["case", case]


def reference_states(case, order="reference", keep=STOPS, lbs=None, ubs=None, costs=None, tag=None):
    """Per instance ``{it: (x, y_eq, y_ineq, draws)}`` of ``dga_cpu`` in the given summation order (cached: do not modify)."""
    key = ("ref", case, order, tuple(keep), tag)
    if key not in _CACHE:
        args, six = batch_case(case)
        costs = six if costs is None else costs
        out = []
        for k in range(costs.shape[0]):
            lb = args[5] if lbs is None else lbs[k]
            ub = args[6] if ubs is None else ubs[k]
            out.append(dga_cpu(costs[k], args[1], args[2], args[3], args[4], lb, ub, nb_max_iter=max(keep) + 1, order=order, keep=keep))
        _CACHE[key] = out
    return _CACHE[key]


# ---- tile remainders: Potts-8, up to 65 instances, every fifth with a tenth of its variables fixed ---------------------------------
REMAINDER_SIZES = (1, 3, 64, 65)
REMAINDER_ITERS = 20


def remainder_batch():
    """``(args, costs, lbs, ubs)`` for 65 instances: ``c (1 + 0.01 k)``; instance k with k % 5 == 0 has ``lb = ub`` on a tenth of
    its variables (per-instance bounds).  A batch of B < 65 is the first B rows."""
    if "remainder" not in _CACHE:
        args, _ = batch_case("potts8")
        c, lb, ub = args[0], args[5], args[6]
        n = c.size
        costs = np.array([c * (1 + 0.01 * k) for k in range(max(REMAINDER_SIZES))])
        lbs, ubs = np.tile(lb, (costs.shape[0], 1)), np.tile(ub, (costs.shape[0], 1))
        for k in range(0, costs.shape[0], 5):
            fixed = np.random.RandomState(100 + k).choice(n, n // 10, replace=False)
            ubs[k, fixed] = lbs[k, fixed]
        _CACHE["remainder"] = (args, costs, lbs, ubs)
    return _CACHE["remainder"]


def remainder_states(order="reference"):
    args, costs, lbs, ubs = remainder_batch()
    return reference_states("potts8", order, keep=(REMAINDER_ITERS - 1,), lbs=lbs, ubs=ubs, costs=costs, tag="remainder")


# ---- an integer-valued LP (the construction of tests/test_gpu_dga.py::integer_lp): sums that do not depend on their order ----------
INT_SHAPE = dict(m=1500, n=5000, per_row=10, m_eq=150, seed=21)
INT_KEEP = (0, 9, 29)


def integer_batch():
    """``(args, costs, lbs, ubs)``: B = 5 integer costs drawn after the LP's own arrays; instances 3 and 4 have 500 variables
    fixed at the feasible point the right-hand sides were built from."""
    if "integer" not in _CACHE:
        import scipy.sparse

        p = INT_SHAPE
        rng = np.random.RandomState(p["seed"])
        m, n, k = p["m"], p["n"], p["per_row"]
        cols = (np.arange(k) * (n // k) + rng.randint(0, n // k, size=(m, k))).astype(np.int32)   # one per stratum: sorted, distinct
        vals = np.round(100 * rng.randn(m, k))
        vals[vals == 0] = 1.0
        a = scipy.sparse.csr_matrix((vals.ravel(), cols.ravel(), np.arange(0, m * k + 1, k)), shape=(m, n))
        lb = rng.randint(-5, 1, size=n).astype(np.float64)
        ub = lb + rng.randint(1, 10, size=n)
        xf = lb + np.floor(rng.rand(n) * (ub - lb + 1))
        ax = a @ xf
        b = ax + rng.randint(0, 50, size=m)
        b[:p["m_eq"]] = ax[:p["m_eq"]]
        c = np.round(100 * rng.randn(n))
        costs = np.round(100 * rng.randn(5, n))
        lbs, ubs = np.tile(lb, (5, 1)), np.tile(ub, (5, 1))
        for inst in (3, 4):
            fixed = rng.choice(n, 500, replace=False)
            lbs[inst, fixed] = xf[fixed]
            ubs[inst, fixed] = xf[fixed]
        args = (c, a[:p["m_eq"]].tocsr(), b[:p["m_eq"]], a[p["m_eq"]:].tocsr(), b[p["m_eq"]:], lb, ub)
        _CACHE["integer"] = (args, costs, lbs, ubs)
    return _CACHE["integer"]


def integer_states(order="reference", on_search=None):
    """Per instance ``{it: (x, y_eq, y_ineq, draws)}`` at ``INT_KEEP``; with ``on_search`` nothing is cached."""
    key = ("integer_ref", order)
    if key in _CACHE and on_search is None:
        return _CACHE[key]
    args, costs, lbs, ubs = integer_batch()
    out = [dga_cpu(costs[k], args[1], args[2], args[3], args[4], lbs[k], ubs[k], nb_max_iter=max(INT_KEEP) + 1, order=order, keep=INT_KEEP,
                   on_search=None if on_search is None else (lambda *a, k=k: on_search(k, *a)))
           for k in range(costs.shape[0])]
    if on_search is None:
        _CACHE[key] = out
    return out
