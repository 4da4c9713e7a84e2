"""numpy restatement of the certificate the Chambolle-Pock list solver stops on (csrc/slp_cp_many.hip,
``CPManyState.set_stop_gap``), fed from ``cp_stop_cpu.oracle_iterates``.

The LP is the one the solver holds: ``K = [A_eq; A_ineq]`` after the one-sided stacking (``ChambollePockPPD._many_problem``, which
touches no library), ``b``, ``c``, ``lb``, ``ub``.  With ``x_t`` and ``y_t = [y_eq; y_ineq]`` after ``t`` whole iterations:

``d_j``        ``c_j + (K^T y_t)_j`` as the next primal half computes it: per column the terms of the equality rows and of the
               inequality rows in two single accumulators, rows increasing, then ``(c + se) + si`` -- the device's bits;
``primal``     ``sum_j c_j x_t,j``;
``bound``      ``sum_j [d_j != 0 ? min(d_j lb_j, d_j ub_j) : 0] - sum_r [y_r != 0 ? y_r b_r : 0]``;
``violation``  ``max(max_{r < m_eq} |(K x_t)_r - b_r|, max_{r >= m_eq} ((K x_t)_r - b_r), 0)`` with ``K x_t`` a single-accumulator
               chain in storage order: the device's bits, and a maximum is exact in any order (a NaN stays, as ``np.max``).

``primal`` and ``bound`` are sums in numpy's order here and in the kernel's fixed order there.  A sum of N products in any order
errs by at most about ``N 2^-53 sum|terms|``, so ``band = 2 (n + m + 3) 2^-52 (sum|c_j x_j| + sum|bound terms| + sum|y_r b_r|)``
covers both orders together with a factor of more than 4.  A check is *decidable* when the decision cannot depend on the order:
the violation alone refuses it, the gap is not finite, or ``|primal - bound|`` is more than 1000 bands from its threshold.

The decision: ``violation <= tol_feas`` and ``|primal - bound| <= tol_gap (1 + |primal| + |bound|)`` with a finite left-hand
side -- a NaN or an infinite gap (``bound = -inf``: a free variable with ``d_j`` of the wrong sign) never stops.

All of the above repeats the device's formula in the device's order on purpose, so an error of the formula itself would stand on
both sides.  Two references that share nothing with it: ``exact_bound``, the bound of a given ``y`` in exact rational arithmetic in
no particular order, and ``highs_optimum``, the LP's optimum from HiGHS, which no lower bound may exceed.
"""
import collections

import numpy as np
import scipy.sparse

import cp_stop_cpu

Certificate = collections.namedtuple("Certificate", "primal bound violation band")
DECIDABLE_BANDS = 1000.0


def held_lp(problem):
    """The LP of the 8-tuple ``problem`` as the solver holds it: a dict of ``c, lb, ub, b, m_eq`` and the entries of ``K`` in
    storage order, ``rows, cols, vals``."""
    from pysparselp_amd.ChambollePockPPD import _many_problem

    c, lb, ub, eq, beq, ineq, b_ineq = _many_problem(0, problem)
    rows, cols, vals, b, m = [], [], [], [], 0
    m_eq = 0 if eq is None else int(eq[3])
    for block, rhs in ((eq, beq), (ineq, b_ineq)):
        if block is None:
            continue
        indptr, indices, data, count = block
        rows.append(m + np.repeat(np.arange(count), np.diff(indptr)))
        cols.append(np.asarray(indices, dtype=np.int64))
        vals.append(np.asarray(data, dtype=np.float64))
        b.append(np.asarray(rhs, dtype=np.float64))
        m += int(count)
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype=dtype)  # noqa: E731
    return dict(c=c, lb=lb, ub=ub, b=cat(b, np.float64), m_eq=m_eq, m=m, rows=cat(rows, np.int64), cols=cat(cols, np.int64),
                vals=cat(vals, np.float64))


def _by_position(keys):
    """The entries grouped by their position inside their row (column) ``keys``, which are non-decreasing: entry ``i`` is in
    group ``p`` when ``p`` entries of the same key come before it.  One group holds at most one entry per key."""
    if keys.size == 0:
        return []
    first = np.concatenate(([True], keys[1:] != keys[:-1]))
    start = np.maximum.accumulate(np.where(first, np.arange(keys.size), 0))
    position = np.arange(keys.size) - start
    return [np.nonzero(position == p)[0] for p in range(int(position.max()) + 1)]


class Restatement:
    """The certificate of one LP; the index work is done once."""

    def __init__(self, problem):
        self.lp = lp = held_lp(problem)
        self.n, self.m = lp["c"].size, lp["m"]
        self.row_groups = _by_position(lp["rows"])   # storage order of K
        order = np.argsort(lp["cols"], kind="stable")   # K^T: rows increasing inside a column
        self.t_rows, self.t_cols, self.t_vals = lp["rows"][order], lp["cols"][order], lp["vals"][order]
        self.col_groups = _by_position(self.t_cols)

    def kx(self, x):
        out = np.zeros(self.m)
        rows, cols, vals = self.lp["rows"], self.lp["cols"], self.lp["vals"]
        for g in self.row_groups:
            out[rows[g]] += vals[g] * x[cols[g]]
        return out

    def direction(self, y):
        lp = self.lp
        se, si = np.zeros(self.n), np.zeros(self.n)
        for g in self.col_groups:
            eq = self.t_rows[g] < lp["m_eq"]
            p = self.t_vals[g] * y[self.t_rows[g]]
            se[self.t_cols[g][eq]] += p[eq]
            si[self.t_cols[g][~eq]] += p[~eq]
        has_eq, has_in = lp["m_eq"] > 0, self.m > lp["m_eq"]
        if has_eq and has_in:
            return (lp["c"] + se) + si
        return lp["c"] + se if has_eq else lp["c"] + si

    def at(self, x, y):
        """``Certificate`` of the iterate ``(x, y)``."""
        lp = self.lp
        with np.errstate(invalid="ignore", over="ignore"):
            d = self.direction(y)
            cx = lp["c"] * x
            terms = np.where(d != 0, np.minimum(d * lp["lb"], d * lp["ub"]), 0.0)
            yb = np.where(y != 0, y * lp["b"], 0.0)
            primal, bound = float(np.sum(cx)), float(np.sum(terms) - np.sum(yb))
            v = self.kx(x) - lp["b"]
            v[:lp["m_eq"]] = np.abs(v[:lp["m_eq"]])
            violation = float(np.max(np.concatenate((v, [0.0]))))
            band = 2.0 * (self.n + self.m + 3) * 2.0 ** -52 * float(np.sum(np.abs(cx)) + np.sum(np.abs(terms)) + np.sum(np.abs(yb)))
        return Certificate(primal, bound, violation, band)


def iterates(problem, nb_iter, x0=None):
    """``cp_stop_cpu.oracle_iterates`` for any LP: one without inequality rows goes through the oracle with an inert row (no
    entry, ``b_upper = 1``), whose multiplier -- always 0.0 -- is dropped."""
    c, a_eq, beq, a_ineq, bl, bu, lb, ub = problem
    if a_ineq is not None and a_ineq.shape[0] > 0:
        return cp_stop_cpu.oracle_iterates(problem, nb_iter, x0)
    through = (c, a_eq, beq, scipy.sparse.csr_matrix((1, np.asarray(c).size)), None, np.ones(1), lb, ub)
    xs, ys = cp_stop_cpu.oracle_iterates(through, nb_iter, x0)
    assert all(y[-1] == 0.0 for y in ys)
    return xs, [y[:-1] for y in ys]


def certificates(problem, xs, ys):
    """``Certificate`` of arrays over ``t = 1 .. T`` from ``[x_0 .. x_T]`` and ``[y_0 .. y_T]``; entry ``t - 1`` belongs to
    iteration ``t``."""
    assert len(xs) == len(ys)
    r = Restatement(problem)
    rows = [r.at(xs[t], ys[t]) for t in range(1, len(xs))]
    out = Certificate(*(np.array(col, dtype=np.float64) for col in zip(*rows))) if rows else Certificate(*(np.zeros(0),) * 4)
    for col in out:
        col.setflags(write=False)
    return out


def decision(primal, bound, violation, tol_gap, tol_feas):
    """The device's decision from three numbers (scalars)."""
    with np.errstate(invalid="ignore"):
        gap = abs(primal - bound)
        return bool(violation <= tol_feas and np.isfinite(gap) and gap <= tol_gap * (1.0 + abs(primal) + abs(bound)))


def bands_from_threshold(cert, t, tol_gap, tol_feas):
    """How many bands ``|primal - bound|`` of iteration ``t`` lies from its threshold; ``inf`` when the decision does not depend on
    the two sums at all (the violation refuses it, or the gap is not finite)."""
    p, b, v, band = (col[t - 1] for col in cert)
    with np.errstate(invalid="ignore"):
        gap = abs(p - b)
        if not v <= tol_feas or not np.isfinite(gap):
            return np.inf
        margin = abs(gap - tol_gap * (1.0 + abs(p) + abs(b)))
    return np.inf if band == 0.0 and margin > 0.0 else (0.0 if band == 0.0 else margin / band)


def decidable(cert, t, tol_gap, tol_feas):
    return bands_from_threshold(cert, t, tol_gap, tol_feas) > DECIDABLE_BANDS


def checks(total, check_every, after=0):
    return [t for t in range(after + 1, total + 1) if t % check_every == 0]


def stopping_iteration(cert, tol_gap, tol_feas, check_every, after=0):
    """The first check iteration ``t > after`` whose decision is to stop, or ``None`` within ``len(cert.primal)``."""
    for t in checks(len(cert.primal), check_every, after):
        if decision(cert.primal[t - 1], cert.bound[t - 1], cert.violation[t - 1], tol_gap, tol_feas):
            return t
    return None


def all_decidable(cert, tol_gap, tol_feas, check_every, total, after=0):
    """Every check the device evaluates in a run of ``total`` iterations is decidable (those up to the stopping iteration)."""
    stop = stopping_iteration(Certificate(*(col[:total] for col in cert)), tol_gap, tol_feas, check_every, after)
    return all(decidable(cert, t, tol_gap, tol_feas) for t in checks(total if stop is None else stop, check_every, after))


def gap_state(cert, tol_gap, tol_feas, check_every, total, after=0, before=(np.inf, -np.inf, np.inf)):
    """``(iterations, stopped, primal, bound, violation)`` as ``CPManyState.gap_state`` reports them for one LP after a run that
    was armed at iteration ``after`` (the last evaluated certificate then ``before``) and asked for ``total`` iterations."""
    t = stopping_iteration(Certificate(*(col[:total] for col in cert)), tol_gap, tol_feas, check_every, after)
    if t is not None:
        return (t, True) + tuple(col[t - 1] for col in cert[:3])
    last = total - total % check_every
    return (total, False) + (tuple(col[last - 1] for col in cert[:3]) if last > after else tuple(before))


_EXACT = {}


def exact_bound(problem, y):
    """The certificate's lower bound ``sum_j min(d_j lb_j, d_j ub_j) - y.b`` with ``d = c + K^T y`` of the LP the solver holds, in
    exact rational arithmetic (every float converts exactly), rounded to a float once at the end: no order of sums, no rounded
    ``d_j``.  ``-inf`` where a variable without a finite bound on that side has ``d_j`` of the wrong sign.  A row without a finite
    side (``b_r = +inf``) has ``y_r = 0`` and no term."""
    from fractions import Fraction

    if id(problem) not in _EXACT:   # the LP's own numbers are converted once
        lp = held_lp(problem)
        exact = {name: [Fraction(v) if np.isfinite(v) else v for v in lp[name].tolist()] for name in ("c", "lb", "ub", "b", "vals")}
        _EXACT[id(problem)] = (problem, dict(exact, rows=lp["rows"].tolist(), cols=lp["cols"].tolist(), m=lp["m"]))
    lp = _EXACT[id(problem)][1]
    ys = [Fraction(float(v)) for v in y]
    assert len(ys) == lp["m"]
    d = list(lp["c"])
    for r, j, v in zip(lp["rows"], lp["cols"], lp["vals"]):
        if ys[r] != 0:
            d[j] += v * ys[r]
    total = Fraction(0)
    for dj, lo, hi in zip(d, lp["lb"], lp["ub"]):
        if dj == 0:
            continue
        side = lo if dj > 0 else hi   # min(d lb, d ub) with lb <= ub
        if not isinstance(side, Fraction):
            return -np.inf
        total += dj * side
    for yr, br in zip(ys, lp["b"]):
        if yr != 0:
            assert isinstance(br, Fraction)
            total -= yr * br
    return float(total)


_HIGHS = {}


def highs_optimum(problem):
    """``scipy.optimize.linprog(method="highs")`` on the 8-tuple ``problem``, cached per LP (by identity; the LP is kept alive):
    the equality rows, and one inequality row per finite side of a two-sided row.  HiGHS's presolve answers "infeasible" where it
    has found the LP infeasible OR unbounded (seen on a feasible, unbounded LP of 65 free-sided variables); an answer of
    "infeasible" is therefore asked again without presolve, and that answer is returned."""
    import scipy.optimize

    if id(problem) not in _HIGHS:
        c, a_eq, beq, a_ineq, bl, bu, lb, ub = problem
        a_ub, b_ub = None, None
        if a_ineq is not None and a_ineq.shape[0] > 0:
            blocks, sides = [a_ineq], [np.asarray(bu, dtype=np.float64)]
            if bl is not None:
                blocks.append(-a_ineq)
                sides.append(-np.asarray(bl, dtype=np.float64))
            rhs = np.concatenate(sides)
            finite = np.isfinite(rhs)
            a_ub, b_ub = scipy.sparse.vstack(blocks).tocsr()[finite], rhs[finite]
        has_eq = a_eq is not None and a_eq.shape[0] > 0
        solve = lambda **options: scipy.optimize.linprog(  # noqa: E731
            c, A_ub=a_ub, b_ub=b_ub, A_eq=a_eq if has_eq else None, b_eq=beq if has_eq else None, bounds=np.column_stack((lb, ub)),
            method="highs", options=options)
        res = solve()
        if res.status == 2:
            res = solve(presolve=False)
        _HIGHS[id(problem)] = (problem, res)
    return _HIGHS[id(problem)][1]


def random_list(seed, count=24):
    """The seeded list of tests/test_gpu_cp_many_gap.py: ``count`` 8-tuples of 1-40 variables and 1-40 rows in the manner of
    ``tools/fuzz_batched.random_lp`` (decimal data, feasible at a point, a mix of row kinds, some infinite bounds, some fixed
    variables); the first four have the edge shapes n = 1, one row, equality rows only, inequality rows only."""
    rng = np.random.RandomState(seed)
    out = []
    dec = lambda size: np.round(rng.randn(size) * 100) / 100  # noqa: E731
    for k in range(count):
        n = 1 if k == 0 else int(rng.randint(1, 41))
        me = int(rng.choice([0, 0, 1, 5, 12]))
        mi = int(rng.randint(1, 41 - me))
        if k == 1:
            me, mi = 0, 1
        if k == 3:
            me = 0
        dens = float(rng.choice([0.2, 0.5, 0.9]))
        ae = scipy.sparse.random(me, n, density=dens, random_state=rng, format="csr")
        ai = scipy.sparse.random(mi, n, density=dens, random_state=rng, format="csr")
        ae.data = dec(ae.nnz) + 0.005
        ai.data = dec(ai.nnz) + 0.005
        xf = dec(n)
        be, bu, bl = ae @ xf, ai @ xf + rng.rand(mi), ai @ xf - rng.rand(mi)
        mode = str(rng.choice(["upper", "two", "mixed"]))
        if mode == "upper":
            bl = None
        elif mode == "mixed":
            bl[rng.rand(mi) < 0.4] = -np.inf
            bu[(rng.rand(mi) < 0.3) & np.isfinite(bl)] = np.inf
        c = dec(n)
        t = np.abs(rng.randn(n)) + 0.1
        t[rng.rand(n) < 0.15] = 0.0
        lb, ub = xf - t, xf + t
        if rng.rand() < 0.3:   # a bound of -inf lasts while a free variable has d_j of the wrong sign: most LPs are boxed
            lb[rng.rand(n) < 0.15] = -np.inf
            ub[rng.rand(n) < 0.15] = np.inf
        eq_only = k == 2 or (me > 0 and rng.rand() < 0.2)
        if k == 2 and me == 0:
            ae = scipy.sparse.csr_matrix(np.round(rng.randn(3, n), 2) + 0.005)
            be, me = ae @ xf, 3
        a_eq, beq = (ae, be) if me else (None, None)
        out.append((c, a_eq, beq, None, None, None, lb, ub) if eq_only else (c, a_eq, beq, ai, bl, bu, lb, ub))
    return out
