"""The LPs of tests/test_gpu_projection_edges.py, built on the host with scipy: the smallest shapes at which each path of
csrc/slp_blocks.hip's row-block projection exists.  tests/test_blocks_cpu_host.py runs every one of them through the exact
reference (tests/blocks_cpu.py) without a GPU and checks that its system is well conditioned.

A case is a dict: ``a`` (scipy CSR, m x n, values rounded to two decimals so that the strip copies find a value dictionary),
``m_eq``, ``b_upper`` (length m, the first ``m_eq`` the equality right-hand sides), ``b_lower`` (length m), ``c``, ``lb``, ``ub``,
``x0`` (a starting point outside the box in places), ``forced`` (the value of SLP_BLOCKS_PRIMAL, or None) and ``exact`` (whether
the dense side is small enough for ``blocks_cpu.project_exact``)."""
import functools

import numpy as np
import scipy.sparse

ONE_GRID = 524288   # threads of the largest launch grid_for() hands out on this part (8 x 256 workgroups of 256)
LONG = 2 * ONE_GRID + 77
BASE_SEED = 38     # of the seeds 1 .. 39 the one whose baseline stays best conditioned with its equality rows scaled (1.9e5)


def sparse_rows(rng, m, n, lo, hi, columns=None, empty_rows=()):
    """m x n CSR with ``lo .. hi`` entries per row drawn over ``columns`` (all when None; a column drawn twice in a row is summed),
    values in [-1, 1] rounded to two decimals, no stored zeros; ``empty_rows`` get none."""
    counts = rng.randint(lo, hi + 1, size=m)
    counts[np.asarray(empty_rows, dtype=np.int64)] = 0
    total = int(counts.sum())
    rows = np.repeat(np.arange(m), counts)
    cols = rng.randint(0, n if columns is None else len(columns), size=total)
    if columns is not None:
        cols = np.asarray(columns)[cols]
    vals = np.round(rng.uniform(-1.0, 1.0, size=total), 2)
    vals[vals == 0.0] = 0.01
    a = scipy.sparse.coo_matrix((vals, (rows, cols)), shape=(m, n)).tocsr()
    a.data = np.round(a.data, 2)
    a.eliminate_zeros()
    a.sort_indices()
    return a


def lp_around(rng, a, m_eq, no_lower=1.0 / 3.0, fixed=5, open_box=0.0):
    """Vectors of an LP over ``a`` around a point inside the box: two-sided rows, a share ``no_lower`` with ``b_lower = -inf``,
    ``fixed`` rows with ``b_lower = b_upper``; a share ``open_box`` of the variables without bounds."""
    m, n = a.shape
    xf = rng.uniform(-0.5, 0.5, size=n)
    ax = a @ xf
    b_upper = ax + rng.rand(m)
    b_upper[:m_eq] = ax[:m_eq]
    b_lower = np.where(rng.rand(m) < no_lower, -np.inf, ax - rng.rand(m))
    ineq = np.arange(m_eq, m)
    if fixed and ineq.size:
        rows = rng.choice(ineq, size=min(fixed, ineq.size), replace=False)
        b_lower[rows] = b_upper[rows]
    b_lower[:m_eq] = b_upper[:m_eq]
    lb, ub = -rng.rand(n), rng.rand(n)
    free = rng.rand(n) < open_box
    lb[free], ub[free] = -np.inf, np.inf
    return {"a": a, "m_eq": int(m_eq), "b_upper": b_upper, "b_lower": b_lower, "c": rng.randn(n), "lb": lb, "ub": ub,
            "x0": 1.5 * rng.randn(n), "forced": None, "exact": True}


def _small(seed, n, m, m_eq, forced=None, **kw):
    rng = np.random.RandomState(seed)
    case = lp_around(rng, sparse_rows(rng, m, n, 1, 12), m_eq, **kw)
    case["forced"] = forced
    return case


def _empty(seed):
    """40 columns without entries -- among them some with a cost and a finite bound, which the unused-column rule moves until the
    bound stops them, and some without bounds -- and 10 inequality rows without entries."""
    rng = np.random.RandomState(seed)
    n, m, m_eq = 300, 200, 60
    empty_cols = rng.choice(n, size=40, replace=False)
    keep = np.setdiff1d(np.arange(n), empty_cols)
    a = sparse_rows(rng, m, n, 1, 12, columns=keep, empty_rows=rng.choice(np.arange(m_eq, m), size=10, replace=False))
    case = lp_around(rng, a, m_eq)
    case["c"][empty_cols[:10]] = 0.0
    case["lb"][empty_cols[10:20]], case["ub"][empty_cols[10:20]] = -np.inf, np.inf
    case["empty_cols"] = empty_cols
    return case


def _long_variables(seed):
    rng = np.random.RandomState(seed)
    return lp_around(rng, sparse_rows(rng, 40, LONG, 12, 12), 12)


def _long_rows(seed):
    rng = np.random.RandomState(seed)
    return lp_around(rng, sparse_rows(rng, LONG, 30, 1, 2), 0)


def _long_slacks(seed):
    """Too many rows for the dense dual system, and equality rows, so no primal form: no exact reference.  300 equality rows over
    200 variables cannot have full rank: ``b_eq = A_eq x`` for a point x, so the system is singular but consistent, and conjugate
    gradients from zero converge on it -- in about 500 steps per projection (12 entries per equality row, one per inequality row:
    with 2 to 4 everywhere the first projection alone takes 1277), which is why this case runs with a step limit of 2000."""
    rng = np.random.RandomState(seed)
    a = scipy.sparse.vstack([sparse_rows(rng, 300, 200, 12, 12), sparse_rows(rng, ONE_GRID + 77, 200, 1, 1)]).tocsr()
    case = lp_around(rng, a, 300)
    case["exact"] = False
    return case


def _csrless(seed):
    rng = np.random.RandomState(seed)
    n, m, m_eq = 3000, 4000, 300
    empty_cols = rng.choice(n, size=50, replace=False)
    a = sparse_rows(rng, m, n, 3, 6, columns=np.setdiff1d(np.arange(n), empty_cols))
    case = lp_around(rng, a, m_eq)
    case["exact"] = False
    case["empty_cols"] = empty_cols
    return case


def _scaled(seed):
    """The baseline with its equality rows scaled by 1, 10, 100 in turn (``b`` alike): unequal diagonals of ``A A^T``."""
    case = dict(_small(seed, 300, 200, 60))
    m_eq = case["m_eq"]
    scale = np.ones(case["a"].shape[0])
    scale[:m_eq] = 10.0 ** (np.arange(m_eq) % 3)
    case["a"] = scipy.sparse.csr_matrix(scipy.sparse.diags(scale) @ case["a"])
    case["a"].data = np.round(case["a"].data, 2)
    case["a"].sort_indices()
    case["b_upper"] = case["b_upper"] * scale
    case["b_lower"] = case["b_lower"] * scale
    return case


def _step_limits(seed):
    rng = np.random.RandomState(seed)
    return lp_around(rng, sparse_rows(rng, 200, 600, 1, 12), 200)


BUILDERS = {
    "dual_both_kinds": lambda: _small(BASE_SEED, 300, 200, 60),
    "dual_inequalities_only": lambda: _small(2, 300, 120, 0),
    "primal_forced": lambda: _small(2, 300, 120, 0, forced="1"),
    "primal_natural": lambda: _small(3, 120, 300, 0),
    "all_equalities": lambda: _small(4, 300, 100, 100),
    "one_slack": lambda: _small(5, 257, 129, 128),
    "one_equality": lambda: _small(6, 257, 129, 1),
    "empty_columns_and_rows": lambda: _empty(7),
    "open_box": lambda: _small(8, 300, 200, 60, open_box=0.5),
    "long_variables": lambda: _long_variables(9),
    "long_rows": lambda: _long_rows(10),
    "long_slacks_behind_equalities": lambda: _long_slacks(11),
    "csrless": lambda: _csrless(12),
    "scaled_equalities": lambda: _scaled(BASE_SEED),
    "step_limits": lambda: _step_limits(13),
}
EXACT = [name for name in BUILDERS if name not in ("long_slacks_behind_equalities", "csrless")]
TABLE = [name for name in EXACT if name not in ("scaled_equalities", "step_limits")]   # the cases of parts (a) and (b)
JACOBI = ["dual_both_kinds", "dual_inequalities_only", "primal_natural", "scaled_equalities"]


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def lp_args(case):
    """``(a, m_eq, b_lower, b_upper, c, lb, ub)`` as ``blocks_cpu.admm2_exact`` / ``blocks_exact`` take them."""
    return case["a"], case["m_eq"], case["b_lower"], case["b_upper"], case["c"], case["lb"], case["ub"]


def solver_args_of(case):
    """``(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub)`` as the oracle's solvers take them."""
    a, m_eq = case["a"], case["m_eq"]
    return (case["c"], a[:m_eq] if m_eq else None, case["b_upper"][:m_eq] if m_eq else None, a[m_eq:], case["b_lower"][m_eq:],
            case["b_upper"][m_eq:], case["lb"], case["ub"])
