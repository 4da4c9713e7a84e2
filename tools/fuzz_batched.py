"""Randomised cross-check of the batched, list and dual-ascent solver families against their CPU references, bit for bit:
``chambolle_pock_ppd_batch`` / ``chambolle_pock_ppd_many`` against ``oracle.chambolle_pock_ppd``, ``lp_admm_batch`` /
``lp_admm_many`` against ``oracle.lp_admm``, ``DeviceDGA`` / ``DeviceDGABatch`` / ``DeviceDGAMany`` against tests/dga_cpu.py in the reference's order of sums
(up to the iteration to which dga_cpu agrees with itself in its three orders, behind it in the device's own order), each batch instance and list LP
also against the single solver alone, the status bits of the LPs on which dga_cpu raises, and the dual bound against HiGHS.

The LPs have wave / tile / padding sizes (n in 1, 2, 3, 63, 64, 65, 127, 129, 255, 257), an empty row, an empty column, a row of
more than 64 entries, one- / two-sided / mixed rows, infinite and equal bounds, warm starts and odd reporting cadences.

``cp_many_stop`` and ``admm_many_stop`` arm the per-LP stopping test of the two list solvers on the same lists (``set_stop`` /
``stop_state``, ``chambolle_pock_ppd_many_until`` / ``lp_admm_many_until``): the tolerances are the reference step (and residual) of
one LP of the list at a check iteration, so that ``<=`` decides by equality; the stopping iterations, flags, steps and residuals
against the numpy restatements (tests/cp_stop_cpu.py, tests/admm_stop_cpu.py) and every LP's frozen iterate against the oracle's
at that LP's own count, bit for bit.  ``dga_many_stop`` does the same for dual gradient ascent on a list (``DeviceDGAMany.set_stop``
/ ``stop_state``, ``dual_gradient_ascent_many_until``) on the lists of ``dga_many``, against tests/dga_stop_cpu.py on dga_cpu's
states; an LP whose stop (or whose last iteration) lies behind its parity horizon is run but not compared, and such LPs are at
most a quarter of a run.

``cp_many_gap`` and ``cp_batch_gap`` arm the certified stopping test of the Chambolle-Pock list solver and of the batched one
(``set_stop_gap`` / ``gap_state``, ``chambolle_pock_ppd_many_certified`` / ``chambolle_pock_ppd_batch_certified``) on lists and batches
of their own, of the same shapes, in which three LPs of four keep their finite bounds (``random_lp(..., boxed=True)``: with a fifth
of either side infinite the bound is ``-inf`` at every size above a dozen variables and nothing stops).  The tolerances are the
violation (``<=`` decides by equality) and the relative gap, with a margin, of one LP at a check iteration; iterations, flags and
records against the numpy restatement (tests/cp_gap_cpu.py), every frozen iterate against the oracle's at its own count, bit for
bit; an LP with a check too close to its threshold to be decided in another order of sums is run, its stopping iteration not
compared (at most 5 % of a family).  The recorded bound is also checked against the formula in exact rational arithmetic on the
device's own ``y`` and, as a lower bound, against HiGHS.

``admm_batch_stop`` arms the per-instance stopping test of the batched ADMM solver (``ADMMBatchState.set_stop`` / ``stop_state``,
``lp_admm_batch_until``) on batches of its own of 1 to 65 instances and one of 260 (at most nine distinct instances, cycled), in
both forms of the iteration and with tile widths 1 to 64 (``SLP_ADMM_BATCH_FORM``, ``SLP_ADMM_BATCH_TILE``): the tolerances are the
restated residual and step of one instance at a check iteration; ``stop_state`` against tests/admm_batch_stop_cpu.py, also armed
in mid-life, armed again and turned off, and every instance's ``x`` and ``lambda`` against the oracle's at its own count, bit for
bit.  No instance is left out.

``dga_batch_stop`` arms the per-instance stopping test of the batched dual gradient ascent (``DeviceDGABatch.set_stop`` /
``stop_state``, ``dual_gradient_ascent_batch_until``) on batches of its own of 1 to 65 instances and one of 260 (at most nine distinct
instances, cycled: identical data under different cut-offs; in every third batch one constructed frozen instance), on all three
paths.  The yardstick is the CPU, not the unarmed device: the step curve from dga_cpu's multipliers and the bound curve from
``dga_cpu.device_energy``, the report's order of sums restated in numpy.  The tolerance is the restated step of one instance at a
check; the cut-offs are, per instance, none, the restated bound of its own curve at a check (``>=`` decides by equality), the next
float above it, or one the curve never reaches.  Armed from creation, and on the fused path also armed in mid-life, armed again with
other cut-offs and another cadence and turned off: ``stop_state`` against tests/dga_batch_stop_cpu.py with its types, every
instance's x, y, tie draws and flags against dga_cpu at its own count and ``report()[k, 0]`` against ``device_energy`` there, bit for
bit, a record that met its cut-off against HiGHS.  An instance that neither stops inside its parity horizon nor has a horizon that
covers the run -- those on which dga_cpu raises before they stop among them -- is run as a neighbour, not compared; such
instance-schedules are at most a quarter of a run.  One more batch of three instances has 65533 variables: the last workgroup of
the bound's column pass holds terms only from 65281 on.

    python tools/fuzz_batched.py [--cases 24] [--seed 0]
        [--family cp_batch,cp_many,admm_batch,admm_many,dga,dga_batch,dga_many,cp_many_stop,admm_many_stop,dga_many_stop,
                  cp_many_gap,cp_batch_gap,admm_batch_stop,dga_batch_stop]

The generators and the CPU references need no GPU (tests/test_fuzz_batched_host.py checks on them that the GPU runs compare what
they claim to); the ``run_*`` functions need one."""
import argparse
import contextlib
import os
import sys

import numpy as np
import scipy.optimize
import scipy.sparse

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from dga_cpu import dga_cpu, dual_argmin  # noqa: E402

EDGE_N = (1, 2, 3, 63, 64, 65, 127, 129, 255, 257)
BATCH_SIZES = (1, 2, 3, 7)
CADENCES = (1, 7, 10, 10 ** 9)
ENERGY_TOL = dict(rtol=1e-9, atol=1e-9)   # the project's bar for the reports' fixed-order sums (tests/test_gpu_cp_batch.py)
CP_TILE_EDGE, ADMM_TILE_EDGE, DGA_TILE_EDGE = 65, 17, 65   # the remainder sizes of the families' own tile-edge tests
LONG_LIST = 260    # more LPs than compute units (256), by cycling
DGA_ITERS = 40
DGA_STOPS = (0, 9, DGA_ITERS - 1)
STATUS_BITS = {"negative step": 1, "empty breakpoint set": 2, "never changes sign": 16}
STOP_EXTRA, STOP_EVERY = 20, (1, 3, 10)   # a stopping list runs 20 iterations longer than its list; the cadences of the test
CP_STOP_OFFSET, ADMM_STOP_OFFSET = 8000, 7000   # the stopping draws' generators: RandomState(seed + offset)
# the same for the dual-ascent lists, which run their DGA_ITERS iterations.  The offset: 6000 was tried first and leaves 138 of the
# 368 LPs of TEST_SEED / TEST_CASES out (the 260-LP list draws cadence 10 there, and a third of its LPs have a parity horizon of one
# iteration); 6027 is the smallest offset from there on that satisfies DGA_STOP_LEFT_OUT on the CPU (51 of 368 left out)
DGA_STOP_OFFSET, DGA_STOP_EVERY = 6027, (1, 2, 5, 10)
DGA_STOP_LEFT_OUT = 0.25   # the largest share of the LPs of a run that may lie behind their parity horizon (not compared)
STOP_AFTER_OFFSET = 500   # on top of them: the generator of ``after``, so that the test's own draws do not depend on it
# the stopping test of the batched ADMM solver (``admm_batch_stop``): batches of their own from RandomState(seed + offset), at most
# ADMM_BATCH_DISTINCT distinct instances each (a larger batch cycles them), ``large_case`` with LONG_LIST instances; every case draws
# one tile width.  The offset: 11000 was tried first and draws no batch of one instance for TEST_SEED / TEST_CASES (it meets every other
# condition of tests/test_fuzz_batched_host.py); 11001 is the smallest offset from there on that meets them all on the CPU
ADMM_BATCH_STOP_OFFSET = 11001
ADMM_BATCH_STOP_SIZES, ADMM_BATCH_DISTINCT, ADMM_BATCH_WIDTHS = (1, 2, 3, 5, 8, 17, 33, 65), 9, (2, 4, 8, 16, 32)
# the stopping test of the batched dual ascent (``dga_batch_stop``): batches of their own from RandomState(seed + offset), at most
# DGA_BATCH_DISTINCT distinct instances each (a larger batch cycles them), ``large_case`` with LONG_LIST instances; DGA_ITERS
# iterations, the cadences of DGA_STOP_EVERY, the cap DGA_STOP_LEFT_OUT on the instance-schedules behind their parity horizon.
# The offset: 12000 was tried first; 12010 is the smallest offset from there on that meets every condition of
# tests/test_fuzz_dga_batch_stop_host.py for TEST_SEED / TEST_CASES on the CPU.  Of the ten before it nine compare no instance at one
# of the sizes n = 1, 2, 3 (the batches of cases 0 .. 2 have 1, 2 and 3 instances, and so small an LP often leaves its parity horizon
# or raises within a few iterations), 12003, 12006, 12007 and 12008 also break the cap (the batch of 260 lies mostly behind its
# horizons there; 12006 misses nothing else), 12000 and 12007 decide by equality in too few cases, 12003 and 12005 stop no instance
# over an LP without inequality rows
DGA_BATCH_STOP_OFFSET = 12010
DGA_BATCH_STOP_SIZES, DGA_BATCH_DISTINCT = (1, 2, 3, 5, 8, 17, 33, 64, 65), 9
DGA_BATCH_STOP_LARGE_N = 65536 - 3   # ``dga_batch_stop_large_case``: the largest size ``dga_cpu.device_energy`` restates is 65536
# the certified stopping test (``cp_many_gap`` / ``cp_batch_gap``): the generators of the lists and of the batches, and on top of
# them those of the coin that boxes an LP (with probability GAP_BOXED) and of the test's own draws.  The lists' offset 9000 meets
# the conditions of tests/test_fuzz_batched_host.py at once.  The batches': 10000 was tried first; 10109 is the smallest offset from
# there on that meets them on the CPU.  Of the 109 before it 91 draw an instance that HiGHS calls infeasible (``batch_of`` moves
# the right-hand sides of the equality rows by 0.01 N(0, 1), which a block of 5 or 12 rows on few variables does not survive), the
# 14 miss an edge size among the LPs with a finite bound, and 4 lack stopping or running instances of one of the kinds
CP_GAP_OFFSET, CP_BATCH_GAP_OFFSET = 9000, 10109
GAP_BOX_OFFSET, GAP_DRAW_OFFSET, GAP_BOXED = 250, 750, 0.75
NEVER_TOL = (1e-2, 1e-2)   # the tolerances of a case none of whose LPs has a finite bound in the last two thirds of its horizon
GAP_LEFT_OUT = 0.05   # the largest share of the entries of a family that may have an undecidable check (run, not compared)
# how far HiGHS's own tolerances may put its optimum below a valid bound, relative to 1 + |optimum|: ten times the largest excess of
# the restatement's finite bounds over the optimum on the draws of TEST_SEED / TEST_CASES, at least ENERGY_TOL's 1e-9.  Measured on
# the CPU: lists 0.0 over 4469 finite records, batches 0.0 over 6245 -- so the floor, 1e-9
HIGHS_ALLOWANCE = 1e-9
# the final records (of the entries that are compared) with a finite bound over an exact -inf, on the restatement
CP_GAP_ROUNDED_TO_ZERO, CP_BATCH_GAP_ROUNDED_TO_ZERO = 0, 0
TEST_SEED, TEST_CASES = 20, 24  # what tests/test_gpu_fuzz_batched.py runs and tests/test_fuzz_batched_host.py checks


# ---- generators ----------------------------------------------------------------------------------------------------------------

def _decimal(rng, size):
    return np.round(rng.randn(size) * 100) / 100


def random_lp(rng, family, n=None, boxed=False):
    """A small LP as a dict ``c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0`` (``a_eq`` None without equality rows), feasible
    at a point ``xf``.  ``family``: ``"cp"`` (any rows; now and then equality rows only), ``"admm"`` (always an inequality block),
    ``"dga"`` (one-sided rows, finite bounds, no start).  ``n``: the number of variables, drawn when None.  Stored values are
    multiples of 0.01 plus 0.005: no stored zero.  ``boxed``: the LP keeps the finite ``lb``, ``ub`` it has before a fifth of
    either side is made infinite; the draws consumed are the same, so nothing else about the LP changes."""
    drawn = int(rng.choice(EDGE_N)) if rng.rand() < 0.5 else int(rng.randint(2, 71))
    n = drawn if n is None else n
    me = int(rng.choice([0, 0, 1, 5, 12]))
    mi = int(rng.randint(1, 91))
    dens = float(rng.choice([0.05, 0.2, 0.5]))
    ae = scipy.sparse.random(me, n, density=dens, random_state=rng, format="lil")
    ai = scipy.sparse.random(mi, n, density=dens, random_state=rng, format="lil")
    empty_row = int(rng.randint(0, mi)) if mi > 1 else None
    # a row of more than 64 entries takes every column at n = 65: no empty column there
    empty_col = int(rng.randint(0, n)) if n > 1 and n != 65 else None
    if n > 64:
        long_row = 0 if mi == 1 else int(rng.choice([r for r in range(mi) if r != empty_row]))
        cols = np.array([j for j in range(n) if j != empty_col])
        ai[long_row, rng.choice(cols, size=int(rng.randint(65, cols.size + 1)), replace=False)] = 1.0
    if empty_row is not None:
        ai[empty_row, :] = 0
    if empty_col is not None:
        ai[:, empty_col] = 0
        ae[:, empty_col] = 0
    ae, ai = ae.tocsr(), ai.tocsr()
    ae.eliminate_zeros()
    ai.eliminate_zeros()
    ae.data = _decimal(rng, ae.nnz) + 0.005
    ai.data = _decimal(rng, ai.nnz) + 0.005
    xf = _decimal(rng, n)
    be = ae @ xf
    bu = ai @ xf + rng.rand(mi)
    bl = ai @ xf - rng.rand(mi)
    mode = "upper" if family == "dga" else str(rng.choice(["upper", "two", "mixed"]))
    if mode == "upper":
        bl = None
    elif mode == "mixed":   # every row keeps a finite side
        bl[rng.rand(mi) < 0.4] = -np.inf
        drop = rng.rand(mi) < 0.3
        bu[drop & np.isfinite(bl)] = np.inf
    c = _decimal(rng, n)
    t = np.abs(rng.randn(n)) + 0.1
    t[rng.rand(n) < 0.15] = 0.0    # fixed variables: lb == ub
    lb, ub = xf - t, xf + t
    box = lb.copy(), ub.copy()
    x0 = None
    if family != "dga":
        lb[rng.rand(n) < 0.2] = -np.inf
        ub[rng.rand(n) < 0.2] = np.inf
        x0 = None if rng.rand() < 0.5 else np.round(rng.randn(n), 2)
    eq_only = me > 0 and rng.rand() < (0.25 if family == "cp" else 0.1 if family == "dga" else 0.0)
    if boxed:
        lb, ub = box
    lp = dict(c=c, a_eq=ae if me else None, beq=be if me else None, a_ineq=ai, b_lower=bl, b_upper=bu, lb=lb, ub=ub, x0=x0)
    if eq_only:
        lp.update(a_ineq=None, b_lower=None, b_upper=None)
    return lp


def batch_of(rng, lp, batch, family):
    """``lp`` as ``batch`` instances: ``c`` becomes ``(batch, n)``; instance 0 is the LP as drawn, instance 1 has exact zeros among
    its costs, the others perturb ``c`` and, by coin flip, ``lb`` / ``ub`` (widened, infinite stays infinite), ``x0`` and -- for
    ``family == "cp"`` -- the right-hand sides (the pattern of finite sides stays that of instance 0)."""
    c = lp["c"]
    n = c.size
    cs = np.tile(c, (batch, 1))
    cs[1:] = c * (1 + 0.2 * rng.randn(batch - 1, n)) + 0.05 * rng.randn(batch - 1, n)
    if batch > 1:
        cs[1, ::3] = 0.0
    out = dict(lp, c=cs)
    if batch == 1:
        return out
    if rng.rand() < 0.5:
        lbs, ubs = np.tile(lp["lb"], (batch, 1)), np.tile(lp["ub"], (batch, 1))
        lbs[1:] -= 0.1 * rng.rand(batch - 1, n)
        ubs[1:] += 0.1 * rng.rand(batch - 1, n)
        out.update(lb=lbs, ub=ubs)
    if rng.rand() < 0.5:
        x0 = np.tile(np.zeros(n) if lp["x0"] is None else lp["x0"], (batch, 1))
        x0[1:] += np.round(0.1 * rng.randn(batch - 1, n), 3)
        out["x0"] = x0
    if family == "cp" and rng.rand() < 0.5:
        if lp["a_eq"] is not None:
            bes = np.tile(lp["beq"], (batch, 1))
            bes[1:] += 0.01 * rng.randn(batch - 1, bes.shape[1])
            out["beq"] = bes
        if lp["a_ineq"] is not None:
            bus = np.tile(lp["b_upper"], (batch, 1))
            bus[1:] += 0.01 * rng.rand(batch - 1, bus.shape[1])
            out["b_upper"] = bus
            if lp["b_lower"] is not None:
                bls = np.tile(lp["b_lower"], (batch, 1))
                bls[1:] -= 0.01 * rng.rand(batch - 1, bls.shape[1])
                out["b_lower"] = bls
    return out


def of_instance(args, k):
    """``((c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub), x0)`` of instance ``k`` of a batch (or of a single LP: ``c`` 1-D)."""
    pick = lambda v: v if (v is None or np.ndim(v) == 1) else v[k]  # noqa: E731
    return ((pick(args["c"]), args["a_eq"], pick(args["beq"]), args["a_ineq"], pick(args["b_lower"]), pick(args["b_upper"]),
             pick(args["lb"]), pick(args["ub"])), pick(args["x0"]))


def edge_n(case):
    """Cases 0 .. 9 of every family have the sizes of ``EDGE_N`` in turn, so that every family meets every edge; None: drawn."""
    return EDGE_N[case] if case < len(EDGE_N) else None


def large_case(cases):
    """The case that carries a family's large instance -- the tile-edge batch, the list longer than 256: the first behind the
    forced edge sizes, or the last."""
    return min(len(EDGE_N), cases - 1)


def batch_sizes(rng, cases, edge, among=BATCH_SIZES):
    """One size per case from ``among``; ``large_case`` has the family's tile-edge size."""
    sizes = [int(rng.choice(among)) for _ in range(cases)]
    sizes[large_case(cases)] = edge
    return sizes


def cp_batch_cases(cases, seed):
    """``[(args, iterations, cadence)]`` of ``run_cp_batch``."""
    rng = np.random.RandomState(seed)
    sizes = batch_sizes(rng, cases, CP_TILE_EDGE)
    return [(batch_of(rng, random_lp(rng, "cp", edge_n(case)), b, "cp"), int(rng.randint(1, 61)), int(rng.choice(CADENCES)))
            for case, b in enumerate(sizes)]


def admm_batch_cases(cases, seed):
    """``[(args, iterations, cadence)]`` of ``run_admm_batch``: always an inequality block, finite costs, shared right-hand sides."""
    rng = np.random.RandomState(seed + 1000)
    sizes = batch_sizes(rng, cases, ADMM_TILE_EDGE)
    return [(batch_of(rng, random_lp(rng, "admm", edge_n(case)), b, "admm"), int(rng.randint(1, 61)), int(rng.choice(CADENCES)))
            for case, b in enumerate(sizes)]


def cp_many_cases(cases, seed):
    """``[(lps, iterations, cadence)]`` of ``run_cp_many``: lists of 1 to 9 LPs of different shapes (the first LP of cases 0 .. 9 has the
    edge sizes in turn); ``large_case`` cycles its LPs to ``LONG_LIST`` entries."""
    rng = np.random.RandomState(seed + 2000)
    out = []
    for case in range(cases):
        lps = [random_lp(rng, "cp", edge_n(case) if k == 0 else None) for k in range(int(rng.randint(1, 10)))]
        if case == large_case(cases):
            lps = [lps[k % len(lps)] for k in range(LONG_LIST)]
        out.append((lps, int(rng.randint(1, 61)), int(rng.choice(CADENCES))))
    return out


def admm_many_cases(cases, seed):
    """``[(lps, iterations, cadence)]`` of ``run_admm_many``: lists of 1 to 9 LPs of different shapes, each with an inequality block
    (the first LP of cases 0 .. 9 has the edge sizes in turn); ``large_case`` cycles its LPs to ``LONG_LIST`` entries.  A generator of
    its own: no other family's draws depend on it."""
    rng = np.random.RandomState(seed + 5000)
    out = []
    for case in range(cases):
        lps = [random_lp(rng, "admm", edge_n(case) if k == 0 else None) for k in range(int(rng.randint(1, 10)))]
        if case == large_case(cases):
            lps = [lps[k % len(lps)] for k in range(LONG_LIST)]
        out.append((lps, int(rng.randint(1, 61)), int(rng.choice(CADENCES))))
    return out


# ---- the per-LP stopping test of the list solvers: draws and what the restatement expects -----------------------------------------

class StopRef:
    """The CPU reference of one LP of a stopping list (never modified): the oracle's iterates ``xs[t]`` and ``duals[t]`` after ``t = 0
    .. total`` iterations (Chambolle-Pock: ``x_t``, ``[y_eq; y_ineq]_t``; ADMM: ``x_t`` over all ``N`` columns, ``lambda_t``;
    ``xs[0]`` of ADMM is the stored start), the restatement's ``curves`` -- ``(step,)`` or ``(residual, step)``, entry ``t - 1`` of
    iteration ``t`` -- the oracle's ``reports`` at the list's cadence over the same horizon, and ``eq_only``."""

    def __init__(self, xs, duals, curves, reports, eq_only=False):
        self.xs, self.duals, self.curves, self.reports, self.eq_only = xs, duals, curves, reports, eq_only


class StopCase:
    """One list with its stopping test: ``lps`` (``problems``, ``x0``), the list's own ``its`` and report cadence ``plot``, the
    horizon ``total = 20 + its``, the cadence ``every`` of the test, the tolerances ``tol`` (a tuple: the reference curves of LP
    ``k_star`` at iteration ``t_star``), ``after`` (the unarmed iterations of the run that is armed in mid-life) and one ``StopRef``
    per distinct LP (``ref(k)``)."""

    def __init__(self, family, lps, its, plot, rng, rng_after):
        import admm_stop_cpu
        import cp_stop_cpu

        self.family, self.lps, self.its, self.plot = family, lps, its, plot
        self.problems = [of_instance(lp, 0)[0] for lp in lps]
        self.x0 = [lp["x0"] for lp in lps]
        self.total = total = STOP_EXTRA + its
        self.every = int(rng.choice(STOP_EVERY))
        checks = [t for t in range(1, total + 1) if t % self.every == 0 and t >= total // 3]
        self.t_star = int(rng.choice(checks))
        self.k_star = int(rng.randint(len(lps)))
        self.after = int(rng_after.randint(1, max(1, total // 3 - 1) + 1))
        self._stop_cpu = cp_stop_cpu if family == "cp" else admm_stop_cpu
        self._refs = {}
        for k, lp in enumerate(lps):   # a cycled list repeats its LPs: one reference each
            if id(lp) not in self._refs:
                self._refs[id(lp)] = (cp_stop_reference if family == "cp" else admm_stop_reference)(self.problems[k], self.x0[k], total, plot)
        self.tol = tuple(float(curve[self.t_star - 1]) for curve in self.ref(self.k_star).curves)

    def ref(self, k):
        return self._refs[id(self.lps[k])]

    def distinct(self):
        return len(self._refs)

    def want(self, after=0):
        """The restatement's ``stop_state`` columns over the list's entries after ``total`` iterations, the test armed after
        ``after`` of them: ``(iterations, stopped, step)`` / ``(iterations, stopped, residual, step)``."""
        rows = {key: self._stop_cpu.stop_state(*ref.curves, *self.tol, self.every, self.total, after=after) for key, ref in self._refs.items()}
        return tuple(np.array(col) for col in zip(*[rows[id(lp)] for lp in self.lps]))


def cp_stop_reference(problem, x0, total, plot):
    """``StopRef`` of one Chambolle-Pock LP.  An LP without inequality rows goes through the oracle with the inert row of
    ``cp_reference``; that row's multiplier (always 0.0) is dropped, so its dual maximum runs over the equality rows alone."""
    import cp_stop_cpu

    c, a_eq, beq, a_ineq, bl, bu, lb, ub = problem
    eq_only = a_ineq is None
    through = (c, a_eq, beq, scipy.sparse.csr_matrix((1, c.size)), None, np.ones(1), lb, ub) if eq_only else problem
    xs, ys = cp_stop_cpu.oracle_iterates(through, total, x0)
    if eq_only:
        assert all(y[-1] == 0.0 for y in ys)
        ys = [y[:-1] for y in ys]
    with np.errstate(invalid="ignore"):   # an energy of the reports over an infinite bound
        reports = cp_reference(problem, x0, total, plot)[0]
    return StopRef(xs, ys, (cp_stop_cpu.steps_of(xs, ys),), reports, eq_only)


def admm_stop_reference(problem, x0, total, plot):
    """``StopRef`` of one ADMM LP: the curves of ``admm_stop_cpu.oracle_curves``, the iterates and the reports of one more run of
    the oracle (``total + 1`` sweeps: call ``i`` of its hook sees ``x_{i+1}`` and ``lambda_i``)."""
    import admm_stop_cpu
    from oracle import oracle

    curves = admm_stop_cpu.oracle_curves(problem, total, x0)
    xs, lams, rec = [np.array(oracle.admm_setup(*problem, x0)["x0"], dtype=np.float64, copy=True)], [], _Reports()

    def hook(i, x, x_all, lam):
        xs.append(np.array(x_all, copy=True))
        lams.append(np.array(lam, copy=True))

    oracle.lp_admm(*problem, x0=x0, nb_iter=total, nb_iter_plot=plot, callback_func=rec, iterate_hook=hook)
    assert len(lams) == total + 1 and np.array_equal(admm_stop_cpu.curves_of(xs[:total + 1], curves[0])[1], curves[1], equal_nan=True)
    if rec.it[-1] == total:   # the driver's horizon is nb_iter = total - 1: no report at index total
        for store in (rec.it, rec.x, rec.e1, rec.e2, rec.veq, rec.vineq):
            store.pop()
    return StopRef(xs[:total + 1], lams, curves, rec)


_STOP_CASES = {}


def _stop_cases(family, lists, offset, cases, seed):
    key = (family, cases, seed)
    if key not in _STOP_CASES:
        rng, rng_after = np.random.RandomState(seed + offset), np.random.RandomState(seed + offset + STOP_AFTER_OFFSET)
        _STOP_CASES[key] = [StopCase(family, lps, its, plot, rng, rng_after) for lps, its, plot in lists(cases, seed)]
    return _STOP_CASES[key]


def cp_stop_cases(cases, seed):
    """``[StopCase]`` of ``run_cp_many_stop``: the lists of ``cp_many_cases`` with a stopping test each, drawn from a generator of
    its own; the references are computed once and shared."""
    return _stop_cases("cp", cp_many_cases, CP_STOP_OFFSET, cases, seed)


def admm_stop_cases(cases, seed):
    """``[StopCase]`` of ``run_admm_many_stop``: the lists of ``admm_many_cases`` with a stopping test each."""
    return _stop_cases("admm", admm_many_cases, ADMM_STOP_OFFSET, cases, seed)


class BatchStopCase(StopCase):
    """One batch of ``lp_admm_batch`` with its stopping test: a ``StopCase`` of family ``"admm"`` whose ``lps`` are the instances of
    the batch taken singly.  ``distinct_args`` holds the distinct instances (``batch_of``), ``args`` the ``batch`` instances the
    device gets: instance ``k`` is distinct instance ``k % distinct``, so a larger batch cycles them and shares their references.
    Beyond ``StopCase``'s draws: the tile ``width`` of the forced settings and, for the run with a schedule, ``rearm`` -- a check
    before ``t_star`` (any iteration before it where there is no such check) at which the test is armed again with both
    tolerances halved -- and ``off``, a later iteration at which it is turned off."""

    def __init__(self, distinct_args, batch, its, plot, rng, rng_after):
        distinct = distinct_args["c"].shape[0]
        singles = []
        for j in range(distinct):
            problem, x0 = of_instance(distinct_args, j)
            singles.append(dict(zip(("c", "a_eq", "beq", "a_ineq", "b_lower", "b_upper", "lb", "ub"), problem), x0=x0))
        pick = np.arange(batch) % distinct
        super().__init__("admm", [singles[j] for j in pick], its, plot, rng, rng_after)
        self.distinct_args = distinct_args
        self.args = {name: v[pick] if (name in ("c", "lb", "ub", "x0") and np.ndim(v) == 2) else v for name, v in distinct_args.items()}
        self.width = int(rng.choice(ADMM_BATCH_WIDTHS))
        before = list(range(self.every, self.t_star, self.every)) or list(range(1, self.t_star))
        self.rearm = int(rng.choice(before))
        self.off = int(rng.randint(self.rearm + 1, self.total + 1))

    def curves(self):
        return tuple(self.ref(k).curves for k in range(len(self.lps)))

    def schedule(self):
        """Armed from creation, armed again at ``rearm`` with halved tolerances, off at ``off``."""
        return [(0, *self.tol, self.every), (self.rearm, *(tol / 2 for tol in self.tol), self.every), (self.off, None, None, 1)]

    def want(self, after=0, schedule=None, total=None):
        """``admm_batch_stop_cpu.stop_state`` over the instances after ``total`` iterations (the case's, when None) of a state armed
        by ``schedule`` -- when None: once, with the case's tolerances, after ``after`` iterations."""
        import admm_batch_stop_cpu

        schedule = [(after, *self.tol, self.every)] if schedule is None else schedule
        return admm_batch_stop_cpu.stop_state(self.curves(), schedule, self.total if total is None else total)


def admm_batch_stop_cases(cases, seed):
    """``[BatchStopCase]`` of ``run_admm_batch_stop``: batches made as those of ``admm_batch_cases`` (cases 0 .. 9 at the edge sizes)
    from generators of their own, with 1 to 65 instances and ``LONG_LIST`` in ``large_case``; the references are computed once per
    distinct instance and shared."""
    key = ("admm_batch", cases, seed)
    if key not in _STOP_CASES:
        rng = np.random.RandomState(seed + ADMM_BATCH_STOP_OFFSET)
        rng_after = np.random.RandomState(seed + ADMM_BATCH_STOP_OFFSET + STOP_AFTER_OFFSET)
        out = []
        for case, b in enumerate(batch_sizes(rng, cases, LONG_LIST, ADMM_BATCH_STOP_SIZES)):
            args = batch_of(rng, random_lp(rng, "admm", edge_n(case)), min(b, ADMM_BATCH_DISTINCT), "admm")
            out.append(BatchStopCase(args, b, int(rng.randint(1, 61)), int(rng.choice(CADENCES)), rng, rng_after))
        _STOP_CASES[key] = out
    return _STOP_CASES[key]


def admm_batch_width(form, batch):
    """The tile width the library chooses for a batch ("Batched ADMM")."""
    if form == "tile":
        return 1 if batch <= 256 else 4 if batch <= 1024 else 16
    return 1 if batch == 1 else 4 if batch <= 4 else 16


def admm_batch_stop_settings(width):
    """``(name, SLP_ADMM_BATCH_FORM, SLP_ADMM_BATCH_TILE)`` of the six runs of a case whose drawn tile width is ``width``."""
    return (("default", None, None), ("tile, drawn width", "tile", width), ("levels, drawn width", "levels", width),
            ("tile, width 64", "tile", 64), ("levels, width 64", "levels", 64), ("levels, width 1", "levels", 1))


def stop_tiles(want, width, every):
    """``(mixed, dead)`` of one run, from the restatement's ``want`` and the tile width: the tiles (``width`` consecutive instances)
    that hold a stopped and a running instance at the end, and the tiles that are wholly stopped at least one check before an
    instance of another tile stops or, still running, reaches the end of the run -- such a tile's workgroup returns at once while
    the others work."""
    iterations, stopped = want[0], want[1]
    mixed = dead = 0
    for start in range(0, len(stopped), width):
        mine = np.zeros(len(stopped), dtype=bool)
        mine[start:start + width] = True
        mixed += bool(stopped[mine].any() and not stopped[mine].all())
        dead += bool(stopped[mine].all() and not mine.all() and iterations[~mine].max() >= iterations[mine].max() + every)
    return mixed, dead


# ---- the certified stopping test of the two Chambolle-Pock families: draws and what the restatement expects ------------------------

class GapRef:
    """The CPU reference of one LP (or batch instance) of a certificate case, never modified: ``problem`` and ``x0``, the oracle's
    iterates ``xs[t]`` (``xs[0]`` the start) and ``ys[t]`` after ``t = 0 .. total`` iterations, the restatement ``restated``
    (``cp_gap_cpu.Restatement``) and its ``cert`` (``cp_gap_cpu.Certificate`` of arrays, entry ``t - 1`` of iteration ``t``), the
    oracle's ``reports`` at the case's cadence, ``eq_only``, ``boxed``."""

    def __init__(self, problem, x0, total, plot, boxed):
        import cp_gap_cpu

        self.problem, self.x0, self.boxed, self.eq_only = problem, x0, boxed, problem[3] is None
        with np.errstate(invalid="ignore", over="ignore"):
            self.xs, self.ys = cp_gap_cpu.iterates(problem, total, x0)
            self.cert = cp_gap_cpu.certificates(problem, self.xs, self.ys)
            self.reports = cp_reference(problem, x0, total, plot)[0]
        self.restated = cp_gap_cpu.Restatement(problem)
        for v in self.xs + self.ys:
            v.setflags(write=False)
        self.n, self.warm = problem[0].size, x0 is not None

    def finite_checks(self, every, total, first=1):
        """The check iterations ``first <= t <= total`` at which primal and bound are finite."""
        return [t for t in range(first, total + 1) if t % every == 0 and np.isfinite(self.cert.primal[t - 1]) and np.isfinite(self.cert.bound[t - 1])]

    def highs(self):
        import cp_gap_cpu

        return cp_gap_cpu.highs_optimum(self.problem)


class GapCase:
    """One list (``family == "many"``) or one batch (``"batch"``) with its certified stopping test.  ``entries``: one ``GapRef``
    per LP of the list (a cycled list repeats them) or per instance; ``args`` the batch; ``its`` and ``plot`` the case's own
    iterations and report cadence, ``total = 20 + its`` the horizon, ``every`` the cadence of the test, ``after`` the unarmed
    iterations of the run that is armed in mid-life.  The tolerances ``tol = (tol_gap, tol_feas)`` come from the record of entry
    ``k_star`` at check iteration ``t_star >= total // 3``, drawn among the pairs whose primal and bound are finite there:
    ``tol_feas`` is that record's violation (a maximum, the device's bits: ``<=`` decides by equality), ``tol_gap`` its relative
    gap times ``1 + 2^-20`` plus ``2^-30`` (the sums depend on the order: the margin puts that check far outside the undecidable
    band, the additive term covers a gap of exactly 0).  A case without such a pair has ``k_star = None`` and ``NEVER_TOL``."""

    def __init__(self, family, entries, its, plot, rng, rng_after, args=None):
        self.family, self.entries, self.its, self.plot, self.args = family, entries, its, plot, args
        self.total = total = STOP_EXTRA + its
        self.every = int(rng.choice(STOP_EVERY))
        self.after = int(rng_after.randint(1, max(1, total // 3 - 1) + 1))
        first = next(t for t in range(max(1, total // 3), total + 1) if t % self.every == 0)
        pairs, seen = [], set()
        for k, ref in enumerate(entries):   # a cycled list repeats its LPs: each distinct LP once
            if id(ref) not in seen:
                seen.add(id(ref))
                pairs += [(k, t) for t in ref.finite_checks(self.every, total, first)]
        self.k_star, self.t_star, self.tol = None, first, NEVER_TOL
        if pairs:
            self.k_star, self.t_star = pairs[int(rng.randint(len(pairs)))]
            p, b, v, _ = (float(col[self.t_star - 1]) for col in entries[self.k_star].cert)
            self.tol = (abs(p - b) / (1.0 + abs(p) + abs(b)) * (1.0 + 2.0 ** -20) + 2.0 ** -30, v)

    def distinct(self):
        out = {}
        for ref in self.entries:
            out.setdefault(id(ref), ref)
        return list(out.values())

    def want(self, after=0):
        """The restatement's ``gap_state`` columns over the entries after ``total`` iterations, the test armed after ``after``."""
        import cp_gap_cpu

        rows = {id(ref): cp_gap_cpu.gap_state(ref.cert, *self.tol, self.every, self.total, after=after) for ref in self.distinct()}
        return tuple(np.array(col) for col in zip(*[rows[id(ref)] for ref in self.entries]))

    def keep(self, after=0):
        """Per entry: is every check it evaluates decidable?  The others are run; their stopping iteration is not compared."""
        import cp_gap_cpu

        able = {id(ref): cp_gap_cpu.all_decidable(ref.cert, *self.tol, self.every, self.total, after=after) for ref in self.distinct()}
        return np.array([able[id(ref)] for ref in self.entries])


def _gap_generators(offset, seed):
    return [np.random.RandomState(seed + offset + extra) for extra in (0, GAP_BOX_OFFSET, GAP_DRAW_OFFSET, STOP_AFTER_OFFSET)]


_GAP_CASES = {}


def cp_gap_cases(cases, seed):
    """``[GapCase]`` of ``run_cp_many_gap``: lists shaped as those of ``cp_many_cases`` (the first LP of cases 0 .. 9 at the edge
    sizes, ``large_case`` cycled to ``LONG_LIST``, 1 to 9 LPs otherwise) from a generator of their own; the coin that boxes an LP
    (probability ``GAP_BOXED``), the draws of the test and ``after`` come from three further generators, so that none depends on
    another.  The references are computed once and shared."""
    key = ("many", cases, seed)
    if key not in _GAP_CASES:
        rng, rng_box, rng_draw, rng_after = _gap_generators(CP_GAP_OFFSET, seed)
        out = []
        for case in range(cases):
            lps = []
            for k in range(int(rng.randint(1, 10))):
                boxed = bool(rng_box.rand() < GAP_BOXED)
                lps.append((random_lp(rng, "cp", edge_n(case) if k == 0 else None, boxed=boxed), boxed))
            its, plot = int(rng.randint(1, 61)), int(rng.choice(CADENCES))
            refs = [GapRef(of_instance(lp, 0)[0], lp["x0"], STOP_EXTRA + its, plot, boxed) for lp, boxed in lps]
            if case == large_case(cases):
                refs = [refs[k % len(refs)] for k in range(LONG_LIST)]
            out.append(GapCase("many", refs, its, plot, rng_draw, rng_after))
        _GAP_CASES[key] = out
    return _GAP_CASES[key]


def cp_batch_gap_cases(cases, seed):
    """``[GapCase]`` of ``run_cp_batch_gap``: batches as those of ``cp_batch_cases`` (``batch_of`` over one LP, ``large_case`` with
    ``CP_TILE_EDGE`` instances) from generators of their own; the LP under a batch is boxed, or not, by the same coin."""
    key = ("batch", cases, seed)
    if key not in _GAP_CASES:
        rng, rng_box, rng_draw, rng_after = _gap_generators(CP_BATCH_GAP_OFFSET, seed)
        sizes = batch_sizes(rng, cases, CP_TILE_EDGE)
        out = []
        for case, b in enumerate(sizes):
            boxed = bool(rng_box.rand() < GAP_BOXED)
            args = batch_of(rng, random_lp(rng, "cp", edge_n(case), boxed=boxed), b, "cp")
            its, plot = int(rng.randint(1, 61)), int(rng.choice(CADENCES))
            refs = [GapRef(*of_instance(args, k), STOP_EXTRA + its, plot, boxed) for k in range(b)]
            out.append(GapCase("batch", refs, its, plot, rng_draw, rng_after, args))
        _GAP_CASES[key] = out
    return _GAP_CASES[key]


def gap_final_records(case):
    """Per entry of ``case`` the final record of the run armed from creation, on the restatement: ``(t, Certificate, y_t)`` -- the
    stopping iteration or the last check -- or None before the first check."""
    want = case.want()
    out = []
    for k, ref in enumerate(case.entries):
        t = int(want[0][k]) if want[1][k] else case.total - case.total % case.every
        out.append(None if t < 1 else (t, type(ref.cert)(*(float(col[t - 1]) for col in ref.cert)), ref.ys[t]))
    return out


_GAP_EXACT = {}


def gap_exact_bound(ref, y):
    """``cp_gap_cpu.exact_bound`` of the LP of ``ref`` at ``y``, computed once per ``(LP, y)``: the device's ``y`` is the oracle's bit
    for bit, and a cycled list repeats its LPs."""
    import cp_gap_cpu

    key = (id(ref), y.tobytes())
    if key not in _GAP_EXACT:
        _GAP_EXACT[key] = cp_gap_cpu.exact_bound(ref.problem, y)
    return _GAP_EXACT[key]


def gap_bound_kind(bound, exact, band):
    """A bound in the device's or the restatement's arithmetic against ``cp_gap_cpu.exact_bound`` on the same ``y``: ``"close"``
    (both finite, within ``band``), ``"both -inf"``, ``"rounded to zero"`` (finite over an exact ``-inf``: a rounded ``d_j == 0.0``
    on a free side whose exact ``d_j`` is not zero; counted, no failure), or None: a mismatch."""
    if np.isfinite(bound) and np.isfinite(exact):
        return "close" if abs(bound - exact) <= band else None
    if bound == -np.inf and exact == -np.inf:
        return "both -inf"
    return "rounded to zero" if np.isfinite(bound) and exact == -np.inf else None


def gap_highs_slack(band, opt):
    """How far a bound of rounding band ``band`` may exceed the optimum ``opt`` HiGHS reports (in the manner of
    ``DgaLP.bound_slack``, plus HiGHS's own tolerances)."""
    return band + HIGHS_ALLOWANCE * (1.0 + abs(opt))


_GAP_STATISTICS = {}


def gap_statistics(cases):
    """``dict(entries, lps, stopped, running, left_out, left_out_late, never_lists, unbounded, boxed_never, rounded_to_zero,
    highs_excess, finite_records)`` of a list of ``GapCase`` on the restatement alone -- what tests/test_fuzz_batched_host.py
    asserts on and the GPU runs compare their counts with.  ``rounded_to_zero`` counts the final records of the kept entries;
    ``highs_excess`` is the largest ``(bound - opt) / (1 + |opt|)`` over all finite records of the LPs HiGHS solves."""
    if id(cases) in _GAP_STATISTICS:   # computed once per list of cases
        return dict(_GAP_STATISTICS[id(cases)][1])
    out = dict(entries=0, lps=0, stopped=0, running=0, left_out=0, left_out_late=0, never_lists=0, unbounded=0, boxed_never=0,
               rounded_to_zero=0, highs_excess=-np.inf, finite_records=0)
    for case in cases:
        want, keep = case.want(), case.keep()
        out["entries"] += len(case.entries)
        out["lps"] += len(case.distinct())
        out["stopped"] += int(want[1].sum())
        out["running"] += int((~want[1]).sum())
        out["left_out"] += int((~keep).sum())
        out["left_out_late"] += int((~case.keep(case.after)).sum())
        out["never_lists"] += case.k_star is None
        out["boxed_never"] += sum(ref.boxed and not want[1][k] for k, ref in enumerate(case.entries))
        for ref in case.distinct():
            res = ref.highs()
            finite = np.isfinite(ref.cert.bound)
            out["unbounded"] += res.status == 3
            if res.status == 0 and finite.any():
                out["finite_records"] += int(finite.sum())
                out["highs_excess"] = max(out["highs_excess"], float(np.max(ref.cert.bound[finite] - res.fun)) / (1.0 + abs(res.fun)))
        cache = {}
        for k, (ref, record) in enumerate(zip(case.entries, gap_final_records(case))):
            if record is None or not keep[k]:
                continue
            key = (id(ref), record[0])
            if key not in cache:
                cache[key] = gap_bound_kind(record[1].bound, gap_exact_bound(ref, record[2]), record[1].band)
            out["rounded_to_zero"] += cache[key] == "rounded to zero"
    _GAP_STATISTICS[id(cases)] = (cases, out)
    return dict(out)


# ---- dual gradient ascent: LPs, batches, lists and their CPU references -----------------------------------------------------------

def _integer_dga_args(rng, n=None):
    """The construction of ``integer_lp`` (tests/test_gpu_dga.py) at small size: integer entries ``round(10 N(0, 1))`` (0 -> 1),
    one entry per column stratum, integer bounds (some equal), costs and slacks: every term of the line search's sums is an
    integer, so the search does not depend on their order.  Every other LP is the same construction with entries +-1, bound
    ranges 0 .. 2 and slacks 0 .. 2: the derivative's values are small integers, so it often vanishes at a breakpoint and the
    search takes a tie draw."""
    drawn = int(rng.choice(EDGE_N)) if rng.rand() < 0.5 else int(rng.randint(2, 71))
    n = drawn if n is None else n
    m_eq = int(rng.choice([0, 0, 1, 5, 12]))
    m = m_eq + int(rng.randint(1, 91))
    k = int(min(n, rng.randint(1, 7)))
    unit = rng.rand() < 0.5
    cols = (np.arange(k) * (n // k) + rng.randint(0, n // k, size=(m, k))).astype(np.int32)
    vals = np.round(10 * rng.randn(m, k))
    vals[vals == 0] = 1.0
    if unit:
        vals = np.sign(vals)
    a = scipy.sparse.csr_matrix((vals.ravel(), cols.ravel(), np.arange(0, m * k + 1, k)), shape=(m, n))
    lb = rng.randint(-5, 1, size=n).astype(np.float64)
    ub = lb + rng.randint(0, 3 if unit else 10, size=n)
    xf = lb + np.floor(rng.rand(n) * (ub - lb + 1))
    ax = a @ xf
    b = ax + rng.randint(0, 3 if unit else 50, size=m)
    b[:m_eq] = ax[:m_eq]
    c = np.round((2 if unit else 10) * rng.randn(n))
    if m_eq > 0 and rng.rand() < 0.1:
        return c, a[:m_eq].tocsr(), b[:m_eq], None, None, lb, ub
    return c, a[:m_eq].tocsr(), b[:m_eq], a[m_eq:].tocsr(), b[m_eq:], lb, ub


def _decimal_dga_args(rng, n=None):
    lp = random_lp(rng, "dga", n)
    n = lp["c"].size
    a_eq = lp["a_eq"] if lp["a_eq"] is not None else scipy.sparse.csr_matrix((0, n))
    b_eq = lp["beq"] if lp["beq"] is not None else np.zeros(0)
    return lp["c"], a_eq, b_eq, lp["a_ineq"], lp["b_upper"], lp["lb"], lp["ub"]


def _status_of(error):
    if isinstance(error, AssertionError):
        return "negative step"
    return next(name for name in STATUS_BITS if name in str(error))


def cpu_states(args, order, iters=DGA_ITERS):
    """``({it: (x, y_eq, y_ineq, draws)}, fail)`` of ``dga_cpu`` in the given order of sums: every iteration it completes (key -1:
    the start) and ``fail`` = None or ``(t, name)`` when it raises in iteration ``t`` (0-based: ``t`` iterations are complete)."""
    def run(k):
        return dga_cpu(*args, nb_max_iter=k, order=order, keep=range(k))

    try:
        return run(iters), None
    except (ValueError, AssertionError) as e:
        name = _status_of(e)
    lo, hi = 0, iters   # run(lo) completes, run(hi) raises
    while hi - lo > 1:
        mid = (lo + hi) // 2
        try:
            run(mid)
            lo = mid
        except (ValueError, AssertionError):
            hi = mid
    return run(lo), (lo, name)


def _same_state(p, q):
    return (np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) and p[3] == q[3]
            and ((p[2] is None and q[2] is None) or np.array_equal(p[2], q[2])))


class DgaLP:
    """One LP of the dual-ascent families: ``args`` as ``dga_cpu`` takes them, ``kind`` (``"integer"`` / ``"decimal"``), a name for
    messages, and its CPU reference (never modified):

    ``states``        ``{it: (x, y_eq, y_ineq, draws)}`` in the reference's order of sums, every iteration it completes;
    ``fail``          None (the LP is ``clean``), or ``(t, name)``: dga_cpu raises ``name`` in iteration ``t``;
    ``horizon``       the last iteration the device is compared with ``states`` at: the last complete one at which the orders
                      ``"reference"``, ``"blocked"`` and ``"device"`` agree bit for bit (the rule of tests/golden/make_dga_golden.py).
                      A decimal-valued LP leaves it through a rounding difference of the sums.  An integer-valued one, whose sums
                      are exact, leaves it through equal breakpoints: the derivative inside a group of equal breakpoints depends
                      on the order the sort gives them (``np.argsort`` there, by (alpha, column) on the device), so the search may
                      count a tie draw in one order and not in the other;
    ``device_states`` the same run with ``order="device"``, the CPU model of the device's own sort and sums: what the device is
                      compared with at the stops behind the horizon (``device_fail``: as ``fail``);
    ``status_ok``     the raise itself is comparable: all orders agree up to iteration ``t - 1`` and raise the same error in ``t``."""

    def __init__(self, args, kind, name):
        self.args, self.kind, self.name = args, kind, name
        self._opt = None
        self.single = {}   # path -> result of the single solver (filled by the GPU runs)
        self.rows = args[1].shape[0], (0 if args[3] is None else args[3].shape[0])
        self.states, self.fail = cpu_states(args, "reference")
        self.clean = self.fail is None
        last = DGA_ITERS - 1 if self.clean else self.fail[0] - 1
        self.horizon, same_raise = last, True
        for order in ("blocked", "device"):
            other, other_fail = cpu_states(args, order)
            agree = -1
            while agree < last and agree + 1 in other and _same_state(self.states[agree + 1], other[agree + 1]):
                agree += 1
            self.horizon = min(self.horizon, agree)
            same_raise = same_raise and other_fail == self.fail
        self.device_states, self.device_fail = other, other_fail
        self.status_ok = not self.clean and same_raise and self.horizon == last

    def stops(self):
        """The iterations the device is compared at: 0, 9 and the last of 40 inside the horizon, and the horizon itself."""
        return sorted({s for s in DGA_STOPS if s <= self.horizon} | ({self.horizon} if self.horizon >= 0 else set()))

    def late_stops(self):
        """The stops behind the horizon that the ``"device"`` order completes: compared with ``device_states``."""
        return [s for s in DGA_STOPS if s > self.horizon and s in self.device_states]

    def linprog(self):
        if self._opt is None:
            c, a_eq, b_eq, a_ineq, b_upper, lb, ub = self.args
            self._opt = scipy.optimize.linprog(c, A_ub=a_ineq, b_ub=b_upper, A_eq=a_eq if a_eq.shape[0] else None,
                                               b_eq=b_eq if a_eq.shape[0] else None, bounds=np.column_stack((lb, ub)), method="highs")
        return self._opt

    def bound_slack(self, y_eq, y_ineq):
        """The rounding of the device's dual energy: gamma_(n + m + 2) (sum |c_bar_j| max(|lb_j|, |ub_j|) + sum |y_i b_i|)."""
        c, a_eq, b_eq, a_ineq, b_upper, lb, ub = self.args
        c_bar, _ = dual_argmin(c, a_eq, a_ineq, lb, ub, y_eq, y_ineq)
        k = c.size + sum(self.rows) + 2
        gamma = k * 2.0 ** -53 / (1 - k * 2.0 ** -53)
        terms = np.sum(np.abs(c_bar) * np.maximum(np.abs(lb), np.abs(ub))) + np.sum(np.abs(y_eq * b_eq))
        if a_ineq is not None:
            terms += np.sum(np.abs(y_ineq * b_upper))
        return gamma * terms


_POOLS = {}


def dga_pool(cases, seed):
    """``cases`` batches of the dual-ascent families, alternately integer- and decimal-valued: ``[[DgaLP, ...], ...]``, the LPs of
    one batch over one matrix and one right-hand side.  Instance 0 is the LP as drawn, instance 1 has exact zeros among its
    costs, the others perturb the costs and, by coin flip, widen the bounds (integers stay integers).  Cases 0 .. 9 have the
    edge sizes in turn, ``large_case`` has ``DGA_TILE_EDGE`` instances.  ``run_dga``, ``run_dga_batch`` and ``run_dga_many`` share the pool and its references."""
    key = (cases, seed)
    if key not in _POOLS:
        rng = np.random.RandomState(seed + 3000)
        sizes = batch_sizes(rng, cases, DGA_TILE_EDGE)
        pool = []
        for case, batch in enumerate(sizes):
            kind = ("integer", "decimal")[case % 2]
            args = _integer_dga_args(rng, edge_n(case)) if kind == "integer" else _decimal_dga_args(rng, edge_n(case))
            pool.append([DgaLP(a, kind, f"seed {seed} case {case} ({kind}) instance {k}")
                         for k, a in enumerate(perturbed(rng, args, kind, batch))])
        _POOLS[key] = pool
    return _POOLS[key]


def perturbed(rng, args, kind, batch):
    """``batch`` LPs over the matrix and right-hand sides of ``args``: see ``dga_pool``."""
    c, lb, ub = args[0], args[5], args[6]
    n = c.size
    out = [args]
    for k in range(1, batch):
        if kind == "integer":
            ck = c + np.round((1 if np.max(np.abs(args[1].data), initial=0) <= 1 and np.max(np.abs(c)) < 10 else 3) * rng.randn(n))
            widen = (lambda: rng.randint(0, 3, size=n).astype(np.float64))
        else:
            ck = c * (1 + 0.2 * rng.randn(n)) + 0.05 * rng.randn(n)
            widen = (lambda: 0.1 * rng.rand(n))
        if k == 1:
            ck[::3] = 0.0
        lbk, ubk = lb, ub
        if rng.rand() < 0.5:
            lbk, ubk = lb - widen(), ub + widen()
        out.append((ck,) + tuple(args[1:5]) + (lbk, ubk))
    return out


def dga_lists(cases, seed):
    """``[[DgaLP, ...], ...]``: ``cases`` lists of 1 to 9 LPs of different shapes drawn from the pool; ``large_case`` is cycled to
    ``LONG_LIST`` entries."""
    pool = dga_pool(cases, seed)
    rng = np.random.RandomState(seed + 4000)
    lists = []
    for case in range(cases):
        picks = rng.choice(len(pool), size=min(len(pool), int(rng.randint(1, 10))), replace=False)
        lps = [pool[p][int(rng.randint(0, len(pool[p])))] for p in picks]
        if case == large_case(cases):
            lps = [lps[k % len(lps)] for k in range(LONG_LIST)]
        lists.append(lps)
    return lists


class DgaStopCase:
    """One list of ``dga_lists`` with the tolerance and the cadence of its stopping test, and per LP the restatement:

    ``steps[k]``     ``step_t`` of LP ``k`` for the iterations inside its parity horizon (``horizon + 1`` of them: there dga_cpu's
                     reference order is the device's bit for bit, and dga_cpu has not raised);
    ``want[k]``      ``(iterations, stopped, step)`` as ``stop_state`` must report them after ``DGA_ITERS`` iterations, or None
                     for an LP that is left out: it neither stops inside its horizon nor has a horizon that covers the run, so
                     where it stops is not known from the CPU;
    ``source``       ``(k, t)``: the tolerance is ``steps[k][t - 1]``, ``t`` a check iteration -- ``<=`` decides by equality there."""

    def __init__(self, lps, rng):
        import dga_stop_cpu

        self.lps = lps
        self.steps = [dga_stop_cpu.steps_of({it: lp.states[it] for it in range(-1, lp.horizon + 1)}) for lp in lps]
        self.every = int(DGA_STOP_EVERY[rng.randint(len(DGA_STOP_EVERY))])
        able = [k for k, s in enumerate(self.steps) if s.size >= 1]
        if able and not any(self.steps[k].size >= self.every for k in able):
            self.every = 1
        able = [k for k in able if self.steps[k].size >= self.every]
        self.source, self.tol = None, 1e-2
        if able:
            k = able[int(rng.randint(len(able)))]
            t = self.every * int(rng.randint(1, self.steps[k].size // self.every + 1))
            if np.isfinite(self.steps[k][t - 1]):
                self.source, self.tol = (k, t), float(self.steps[k][t - 1])
        self.want = []
        for lp, steps in zip(lps, self.steps):
            t = dga_stop_cpu.stopping_iteration(steps, self.tol, self.every)
            if t is None and steps.size < DGA_ITERS:
                self.want.append(None)
            else:
                self.want.append(dga_stop_cpu.stop_state(steps, self.tol, self.every, DGA_ITERS))

    def compared(self):
        return [k for k, w in enumerate(self.want) if w is not None]


_DGA_STOP_CASES = {}


def dga_stop_cases(cases, seed):
    """``[DgaStopCase, ...]`` on the lists of ``dga_lists``; the draws of list ``case`` come from ``RandomState(seed +
    DGA_STOP_OFFSET + case)``, so that a list's test does not depend on the lists before it."""
    key = (cases, seed)
    if key not in _DGA_STOP_CASES:
        _DGA_STOP_CASES[key] = [DgaStopCase(lps, np.random.RandomState(seed + DGA_STOP_OFFSET + case))
                                for case, lps in enumerate(dga_lists(cases, seed))]
    return _DGA_STOP_CASES[key]


def dga_stop_statistics(cases, seed):
    """``dict(lps, left_out, stopped, running, lists_with_both, by_equality, longest)`` over the LPs of ``dga_stop_cases`` -- what
    tests/test_fuzz_dga_stop_host.py asserts on and ``run_dga_many_stop`` asserts its cap with."""
    out = dict(lps=0, left_out=0, stopped=0, running=0, lists_with_both=0, by_equality=0, longest=0)
    for case in dga_stop_cases(cases, seed):
        known = [w for w in case.want if w is not None]
        out["lps"] += len(case.lps)
        out["left_out"] += len(case.lps) - len(known)
        out["stopped"] += sum(bool(w[1]) for w in known)
        out["running"] += sum(not w[1] for w in known)
        out["lists_with_both"] += any(w[1] for w in known) and any(not w[1] for w in known)
        out["by_equality"] += case.source is not None and case.want[case.source[0]] is not None and case.want[case.source[0]][2] == case.tol
        out["longest"] = max(out["longest"], len(case.lps))
    return out


# ---- the per-instance stopping test of the batched dual ascent: batches of their own, rules, what the restatement expects ----------

def _frozen_args(rng, args):
    """``args`` with one finite bound of one variable opened to +-inf on the side the start's ``c_bar`` pushes it to (the
    construction of tests/test_gpu_dga_batch.py::_sc50a_with_an_unbounded_instance): ``dual_energy`` of the start is ``-inf``, so
    the instance is frozen at creation.  None when the start's ``c_bar`` is zero everywhere."""
    from dga_cpu import dual_energy

    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = args
    rs = np.random.RandomState(0)
    y_eq = -rs.rand(a_eq.shape[0])
    y_ineq = np.abs(rs.rand(a_ineq.shape[0])) if a_ineq is not None else None
    c_bar, _ = dual_argmin(c, a_eq, a_ineq, lb, ub, y_eq, y_ineq)
    able = np.flatnonzero(c_bar != 0)
    if able.size == 0:
        return None
    j = int(able[rng.randint(able.size)])
    lb, ub = lb.copy(), ub.copy()
    if c_bar[j] < 0:
        ub[j] = np.inf
    else:
        lb[j] = -np.inf
    assert dual_energy(c, a_eq, b_eq, a_ineq, b_upper, lb, ub, y_eq, y_ineq) == -np.inf
    return c, a_eq, b_eq, a_ineq, b_upper, lb, ub


class DgaBatchStopCase:
    """One batch of ``DeviceDGABatch`` with the rules of its stopping test.

    ``lps``           one ``DgaLP`` per instance: instance ``k`` is distinct instance ``k % len(distinct)`` (at most
                      ``DGA_BATCH_DISTINCT`` of them; a larger batch cycles them and shares their references), but for
                      ``frozen_at`` (None, or the position of the constructed frozen instance: its neighbour's data with one
                      bound opened, ``_frozen_args``);
    ``steps(k)``,     the restated curves of instance ``k`` inside its parity horizon, ``horizon + 1`` entries (none for the frozen
    ``bounds(k)``     instance): ``dga_stop_cpu.steps_of`` and ``dga_cpu.device_energy`` on ``lp.states``, once per distinct LP;
    ``every, tol,     the rule of schedule A, armed from creation.  ``source = (k, t)``: ``tol`` is ``steps(k)[t - 1]``, ``t`` a check
    targets``         -- ``<=`` decides by equality (None: no such instance, or no step test).  ``kinds[k] = (kind, t)`` tells where
                      ``targets[k]`` comes from: ``"none"`` (``+inf``), ``"equal"`` (``bounds(k)[t - 1]``: ``>=`` decides by equality),
                      ``"above"`` (``np.nextafter`` of it upward: not met at that check) or ``"never"`` (the curve's maximum + 1);
                      ``both``: the source instance has the cut-off of its own bound at the check of ``tol`` (reason 3);
    ``rules_b``       schedule B: ``(after, tol, targets, every)``, ``(after2, tol / 2 or None, targets2, every2)`` with cut-offs
                      and a cadence drawn afresh, ``(after3, None, None, 1)``: armed in mid-life, armed again, turned off."""

    def __init__(self, no, distinct, batch, frozen_at, frozen_lp, rng):
        import dga_cpu as cpu
        import dga_stop_cpu

        self.no, self.distinct, self.frozen_at = no, distinct, frozen_at
        self.lps = [distinct[k % len(distinct)] for k in range(batch)]
        if frozen_at is not None:
            self.lps[frozen_at] = frozen_lp
        self.frozen = np.array([k == frozen_at for k in range(batch)])
        self._curves = {}
        for lp in distinct + ([] if frozen_lp is None else [frozen_lp]):
            inside = {it: lp.states[it] for it in range(-1, lp.horizon + 1)}
            bounds = np.array([cpu.device_energy(*lp.args, inside[it][1], inside[it][2]) for it in range(lp.horizon + 1)])
            self._curves[id(lp)] = (dga_stop_cpu.steps_of(inside), bounds)
            for curve in self._curves[id(lp)]:
                curve.setflags(write=False)
        live = [k for k in range(batch) if not self.frozen[k]]
        self.every = int(DGA_STOP_EVERY[rng.randint(len(DGA_STOP_EVERY))])
        if not any(self.steps(k).size >= self.every for k in live):
            self.every = 1
        able = [k for k in live if self.steps(k).size >= self.every]
        want_tol, want_targets = no % 5 != 4, no % 5 != 2   # one case of five without a step test, another without cut-offs
        self.source, self.tol, self.both = None, None, False
        pick, at, coin = rng.randint(2 ** 31), rng.rand(), rng.rand()   # consumed in every case: the later draws do not shift
        if want_tol or not able:
            self.tol = 1e-2
            if able:
                k = able[pick % len(able)]
                t = self.every * (1 + int(at * (self.steps(k).size // self.every)))
                if np.isfinite(self.steps(k)[t - 1]):
                    self.source, self.tol = (k, t), float(self.steps(k)[t - 1])
        self.targets, self.kinds = self.draw_targets(rng, self.every) if want_targets or self.tol is None else (None, None)
        if self.targets is not None and self.source is not None and coin < 0.5:
            k, t = self.source
            if np.isfinite(self.bounds(k)[t - 1]):
                self.targets[k], self.kinds[k], self.both = self.bounds(k)[t - 1], ("equal", t), True
        after = int(rng.randint(1, 10))
        after2 = int(rng.randint(after + 1, 26))
        every2 = int(DGA_STOP_EVERY[rng.randint(len(DGA_STOP_EVERY))])
        targets2, self.kinds2 = self.draw_targets(rng, every2)
        after3 = int(rng.randint(after2 + 1, 36))
        self.rules_a = [(0, self.tol, self.targets, self.every)]
        self.rules_b = [(after, self.tol, self.targets, self.every), (after2, None if self.tol is None else self.tol / 2, targets2, every2),
                        (after3, None, None, 1)]
        self._want = {}

    def steps(self, k):
        return self._curves[id(self.lps[k])][0]

    def bounds(self, k):
        return self._curves[id(self.lps[k])][1]

    def draw_targets(self, rng, every):
        """One cut-off per instance of the batch, of one of the four kinds drawn uniformly, on the instance's own curve at a drawn
        check of cadence ``every``; an instance without such a check (the frozen one among them) has none: ``+inf``."""
        kinds = ("none", "equal", "above", "never")
        targets, drawn = np.full(len(self.lps), np.inf), []
        for k in range(len(self.lps)):
            kind, at = kinds[rng.randint(4)], rng.rand()
            bounds = self.bounds(k)
            t = every * (1 + int(at * (bounds.size // every))) if bounds.size >= every else 0
            value = {"none": np.inf, "equal": bounds[t - 1], "above": np.nextafter(bounds[t - 1], np.inf),
                     "never": np.max(bounds) + 1.0}[kind] if t else np.inf
            if not np.isfinite(value):
                kind, t, value = "none", 0, np.inf
            targets[k] = value
            drawn.append((kind, t))
        return targets, drawn

    def schedule(self, name):
        return self.rules_a if name == "A" else self.rules_b

    def want(self, name, total=DGA_ITERS):
        """``(stop_state of dga_batch_stop_cpu, known)`` of schedule ``name`` after ``total`` iterations of the state's life, on the
        curves restricted to the horizons (behind them NaN, which meets nothing).  ``known[k]``: the instance is frozen, stops
        inside its horizon, or its horizon covers the ``total`` iterations -- the others are run as neighbours, not compared."""
        import dga_batch_stop_cpu

        if (name, total) not in self._want:
            pad = lambda v: np.concatenate((v, np.full(max(0, DGA_ITERS - v.size), np.nan)))  # noqa: E731
            batch = range(len(self.lps))
            state = dga_batch_stop_cpu.stop_state([pad(self.steps(k)) for k in batch], [pad(self.bounds(k)) for k in batch],
                                                  self.schedule(name), total, frozen=self.frozen)
            known = self.frozen | state[1] | np.array([self.steps(k).size >= total for k in batch])
            self._want[(name, total)] = (state, known)
        return self._want[(name, total)]

    def phases(self, name):
        """The iteration counts at which a run of schedule ``name`` is compared: A at its end; B when each of its rules is armed
        (the end of the unarmed run and of the first two rules) and at its end."""
        return [DGA_ITERS] if name == "A" else [rule[0] for rule in self.rules_b] + [DGA_ITERS]

    def start_bound(self, k):
        import dga_cpu as cpu

        start = self.lps[k].states[-1]
        return cpu.device_energy(*self.lps[k].args, start[1], start[2])

    def rule_text(self, name):
        rules = "; ".join(f"after {a}: tol {tol!r}, targets {'None' if tg is None else 'given'}, every {ev}" for a, tol, tg, ev in self.schedule(name))
        return f"schedule {name} ({rules}; tol from {self.source})"


_DGA_BATCH_STOP_CASES = {}


def dga_batch_stop_cases(cases, seed):
    """``[DgaBatchStopCase]`` of ``run_dga_batch_stop``: batches of their own from ``RandomState(seed + DGA_BATCH_STOP_OFFSET)``,
    integer- and decimal-valued in turn, cases 0 .. 9 at the edge sizes, the batch sizes of ``DGA_BATCH_STOP_SIZES`` in turn and
    ``LONG_LIST`` in ``large_case``; in every third case, from three instances on, one instance at a drawn position is the constructed
    frozen one.  The rule of case ``i`` comes from ``RandomState(seed + DGA_BATCH_STOP_OFFSET + STOP_AFTER_OFFSET + i)``."""
    key = (cases, seed)
    if key not in _DGA_BATCH_STOP_CASES:
        rng = np.random.RandomState(seed + DGA_BATCH_STOP_OFFSET)
        out = []
        for case in range(cases):
            batch = LONG_LIST if case == large_case(cases) else DGA_BATCH_STOP_SIZES[case % len(DGA_BATCH_STOP_SIZES)]
            kind = ("integer", "decimal")[case % 2]
            args = _integer_dga_args(rng, edge_n(case)) if kind == "integer" else _decimal_dga_args(rng, edge_n(case))
            name = f"seed {seed} case {case} ({kind}, n {args[0].size}) distinct instance "
            distinct = [DgaLP(a, kind, name + str(j)) for j, a in enumerate(perturbed(rng, args, kind, min(batch, DGA_BATCH_DISTINCT)))]
            frozen_at = frozen_lp = None
            if case % 3 == 2 and batch >= 3:
                at = int(rng.randint(batch))
                opened = _frozen_args(rng, distinct[at % len(distinct)].args)
                if opened is not None:
                    frozen_at, frozen_lp = at, DgaLP(opened, kind, name + f"{at % len(distinct)} with a bound opened (frozen)")
                    assert sorted(frozen_lp.states) == [-1] and frozen_lp.horizon == -1
            out.append(DgaBatchStopCase(case, distinct, batch, frozen_at, frozen_lp,
                                        np.random.RandomState(seed + DGA_BATCH_STOP_OFFSET + STOP_AFTER_OFFSET + case)))
        _DGA_BATCH_STOP_CASES[key] = out
    return _DGA_BATCH_STOP_CASES[key]


def dga_batch_stop_large_case(seed):
    """One ``DgaBatchStopCase`` of three integer-valued instances with ``DGA_BATCH_STOP_LARGE_N`` variables (more than the fused
    search takes): the last of the 256 workgroups of the bound's column pass holds terms, which no size below 65281 reaches, and
    the size is no multiple of the workgroup.  Generators of its own, behind those of the rules of the cases."""
    key = ("large", seed)
    if key not in _DGA_BATCH_STOP_CASES:
        rng = np.random.RandomState(seed + DGA_BATCH_STOP_OFFSET + 2 * STOP_AFTER_OFFSET)
        args = _integer_dga_args(rng, DGA_BATCH_STOP_LARGE_N)
        name = f"seed {seed} large case (integer, n {DGA_BATCH_STOP_LARGE_N}) distinct instance "
        distinct = [DgaLP(a, "integer", name + str(j)) for j, a in enumerate(perturbed(rng, args, "integer", 3))]
        _DGA_BATCH_STOP_CASES[key] = DgaBatchStopCase(0, distinct, 3, None, None, np.random.RandomState(seed + DGA_BATCH_STOP_OFFSET + 2 * STOP_AFTER_OFFSET + 1))
    return _DGA_BATCH_STOP_CASES[key]


def dga_batch_stop_statistics(cases, seed):
    """Counts over ``dga_batch_stop_cases`` on the restatement alone -- what tests/test_fuzz_dga_batch_stop_host.py asserts on and
    ``run_dga_batch_stop`` asserts its cap with.  ``instance_schedules`` = ``compared + left_out`` over both schedules;
    ``by_step`` / ``by_bound`` / ``by_both`` / ``running`` split the compared ones by reason; the others are documented there."""
    out = dict(instance_schedules=0, compared=0, left_out=0, by_step=0, by_bound=0, by_both=0, running=0, batches_with_both=0,
               step_by_equality=0, bound_by_equality=0, above_not_met=0, sizes=set(), edge_sizes=set(), stopped_without_ineq=0,
               stopped_without_eq=0, frozen=0, frozen_between=0, b_first_phase=0, b_second_phase=0, b_survive_off=0, twins_apart=0, longest=0,
               idle_batches=0, driver_batches=0)
    for case in dga_batch_stop_cases(cases, seed):
        batch = len(case.lps)
        out["driver_batches"] += case.frozen_at is None and all(lp.clean and lp.device_fail is None for lp in case.lps)
        out["sizes"].add(batch)
        out["longest"] = max(out["longest"], batch)
        out["frozen"] += case.frozen_at is not None
        out["frozen_between"] += case.frozen_at is not None and 0 < case.frozen_at < batch - 1
        for name in ("A", "B"):
            (iterations, stopped, step, bound, reason), known = case.want(name)
            out["instance_schedules"] += batch
            out["compared"] += int(known.sum())
            out["left_out"] += int((~known).sum())
            live = known & ~case.frozen
            for bit, label in ((1, "by_step"), (2, "by_bound"), (3, "by_both")):
                out[label] += int((live & (reason == bit)).sum())
            out["running"] += int((live & ~stopped).sum())
            out["edge_sizes"] |= {case.lps[k].args[0].size for k in np.flatnonzero(live)}
            for k in np.flatnonzero(live & stopped):
                out["stopped_without_ineq"] += case.lps[k].rows[1] == 0
                out["stopped_without_eq"] += case.lps[k].rows[0] == 0
            if name == "B":
                (a1, _, _, _), (a2, _, _, _), (a3, _, _, _) = case.rules_b
                done = iterations[live & stopped]
                out["b_first_phase"] += int(((done > a1) & (done <= a2)).sum())
                out["b_second_phase"] += int(((done > a2) & (done <= a3)).sum())
                out["b_survive_off"] += int(done.size)
                continue
            out["batches_with_both"] += bool((live & stopped).any() and (live & ~stopped).any())
            out["idle_batches"] += bool(known.all() and (stopped | case.frozen).all())
            met = [k for k in np.flatnonzero(live & stopped)]
            out["step_by_equality"] += any(reason[k] & 1 and step[k] == case.tol for k in met)
            out["bound_by_equality"] += any(reason[k] & 2 and bound[k] == case.targets[k] for k in met)
            if case.kinds is not None:   # the check of the cut-off is reached alive, and the bound there lies below it
                out["above_not_met"] += sum(case.kinds[k][0] == "above" and iterations[k] >= case.kinds[k][1]
                                            and case.bounds(k)[case.kinds[k][1] - 1] < case.targets[k] for k in np.flatnonzero(live))
            twins = {}
            for k in met:
                twins.setdefault(id(case.lps[k]), set()).add(int(iterations[k]))
            out["twins_apart"] += sum(len(v) > 1 for v in twins.values())
    return out


def dga_statistics(cases, seed):
    """Per value kind ``dict(drawn, clean, no_crossing, empty, negative, comparable_raises, short_horizon, min_horizon, late)`` over all
    the LPs of the pool -- what tests/test_fuzz_batched_host.py asserts on."""
    out = {}
    for kind in ("integer", "decimal"):
        lps = [lp for batch in dga_pool(cases, seed) for lp in batch if lp.kind == kind]
        names = [lp.fail[1] for lp in lps if lp.fail is not None]
        clean = [lp for lp in lps if lp.clean]
        out[kind] = dict(drawn=len(lps), clean=len(clean), no_crossing=names.count("never changes sign"),
                         empty=names.count("empty breakpoint set"), negative=names.count("negative step"),
                         comparable_raises=sum(lp.status_ok for lp in lps),
                         short_horizon=sum(lp.horizon < 10 for lp in clean), min_horizon=min([lp.horizon for lp in clean], default=-1),
                         late=sum(len(lp.late_stops()) for lp in lps))
    return out


# ---- the GPU runs: helpers -----------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def environment(**values):
    """The switches the library reads when a state is created; None unsets."""
    saved = {name: os.environ.get(name) for name in values}
    try:
        for name, v in values.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = str(v)
        yield
    finally:
        for name, v in saved.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v


def _require(ok, where, layer=None):
    """``layer()`` -- does the single solver agree with the CPU reference on that LP? -- runs only on a mismatch."""
    if not ok:
        raise AssertionError(where + ("" if layer is None else "; " + layer()))


def _pieces(k):
    """``k`` iterations as calls of uneven size."""
    out = []
    for p in (1, 3, 7):
        if k > p:
            out.append(p)
            k -= p
    return out + ([k] if k > 0 else [])


class _Reports:
    """The callback calls of a solver (copies)."""

    def __init__(self):
        self.it, self.x, self.e1, self.e2, self.veq, self.vineq = [], [], [], [], [], []

    def __call__(self, niter, sol, e1, e2, dur, veq, vineq):
        self.it.append(niter)
        self.x.append([np.array(v, copy=True) for v in sol] if isinstance(sol, list) else np.array(sol, copy=True))
        for store, v in ((self.e1, e1), (self.e2, e2), (self.veq, veq), (self.vineq, vineq)):
            store.append(np.array(v, dtype=np.float64, copy=True))


def _compare_reports(got, k, ref, where, layer, vineq=True):
    """Instance / LP ``k`` of the batched reports ``got`` against the reference's ``ref``: x and the maxima bit for bit, the
    energies within ``ENERGY_TOL``."""
    _require(got.it == ref.it, f"{where}: reports at {got.it}, the reference's at {ref.it}")
    for i, it in enumerate(ref.it):
        at = f"{where}, report at iteration {it}"
        _require(np.array_equal(got.x[i][k], ref.x[i]), at + ": x differs", layer)
        _require(got.veq[i][k] == ref.veq[i], at + f": max violated equality {got.veq[i][k]!r} != {ref.veq[i]!r}", layer)
        if vineq:
            _require(got.vineq[i][k] == ref.vineq[i], at + f": max violated inequality {got.vineq[i][k]!r} != {ref.vineq[i]!r}", layer)
        for name, g, r in (("energy1", got.e1[i][k], ref.e1[i]), ("energy2", got.e2[i][k], ref.e2[i])):
            _require(np.allclose(g, r, equal_nan=True, **ENERGY_TOL), at + f": {name} {g!r} != {r!r}", layer)


# ---- Chambolle-Pock ------------------------------------------------------------------------------------------------------------------

def cp_reference(problem, x0, its, plot):
    """``oracle.chambolle_pock_ppd`` on one LP: ``(reports, x, y at the last report point, equalities only?)`` -- y is ``[y_eq;
    y_ineq]`` as the last iteration's report would see it.  An LP without inequality rows gets the inert all-zero row with a
    positive bound of tests/test_gpu_edge_cases.py::test_cp_equalities_only_runs_and_reports (the oracle needs the block)."""
    from oracle import oracle

    c, a_eq, beq, a_ineq, bl, bu, lb, ub = problem
    n = c.size
    eq_only = a_ineq is None
    if eq_only:
        a_ineq, bl, bu = scipy.sparse.csr_matrix((1, n)), None, np.ones(1)
    if a_eq is None:
        a_eq, beq = scipy.sparse.csr_matrix((0, n)), np.zeros(0)
    rec, last = _Reports(), {}

    def hook(niter, x, y_eq, y_ineq):
        if niter == its - 1:
            last["y"] = np.concatenate((np.zeros(0) if y_eq is None else y_eq, np.zeros(0) if (eq_only or y_ineq is None) else y_ineq))
            last["x"] = x.copy()

    x, _ = oracle.chambolle_pock_ppd(c, a_eq, beq, a_ineq, bl, bu, lb, ub, x0=x0, nb_max_iter=its, nb_iter_plot=plot, callback_func=rec,
                                     iterate_hook=hook)
    assert np.array_equal(x, last["x"])
    return rec, x, last["y"], eq_only


def _cp_single_agrees(problem, x0, its, x_ref):
    def layer():
        from pysparselp_amd import ORDER_SEQUENTIAL
        from pysparselp_amd.ChambollePockPPD import chambolle_pock_ppd

        c, a_eq, beq, a_ineq, bl, bu, lb, ub = problem
        if a_ineq is None:
            a_ineq, bu = scipy.sparse.csr_matrix((0, c.size)), np.zeros(0)
        if a_eq is None:
            a_eq, beq = scipy.sparse.csr_matrix((0, c.size)), np.zeros(0)
        x, _ = chambolle_pock_ppd(c, a_eq, beq, a_ineq, bl, bu, lb, ub, x0=x0, nb_max_iter=its, nb_iter_plot=10 ** 9, order=ORDER_SEQUENTIAL)
        return "chambolle_pock_ppd in ORDER_SEQUENTIAL on this LP alone " + ("AGREES" if np.array_equal(x, x_ref) else "DISAGREES") \
            + " with the oracle"
    return layer


def _state_at_last_report(state, its):
    """x and y of a Chambolle-Pock state as the report of iteration ``its - 1`` sees them, reached in uneven calls."""
    for p in _pieces(its - 1):
        state.iterate(p)
    state.primal_step()
    return state.x(), state.y()


def run_cp_batch(cases, seed):
    """``chambolle_pock_ppd_batch`` and ``CPBatchState``: every instance against the oracle.  Returns counts."""
    from pysparselp_amd import CPBatchState, chambolle_pock_ppd_batch
    from pysparselp_amd.ChambollePockPPD import one_sided_system_batch

    counts = dict(batches=0, instances=0, reports=0, equalities_only=0)
    for case, (args, its, plot) in enumerate(cp_batch_cases(cases, seed)):
        batch = args["c"].shape[0]
        rec = _Reports()
        x, _ = chambolle_pock_ppd_batch(args["c"], args["a_eq"], args["beq"], args["a_ineq"], args["b_lower"], args["b_upper"], args["lb"],
                                        args["ub"], x0=args["x0"], nb_max_iter=its, nb_iter_plot=plot, callback_func=rec)
        ineq, b_ineq = (None, None) if args["a_ineq"] is None else one_sided_system_batch(args["a_ineq"], args["b_lower"], args["b_upper"])
        state = CPBatchState(args["c"], args["a_eq"], args["beq"], ineq, b_ineq, args["lb"], args["ub"], args["x0"], 1, 1)
        try:
            xs, ys = _state_at_last_report(state, its)
        finally:
            state.close()
        for k in range(batch):
            problem, x0 = of_instance(args, k)
            ref, x_ref, y_ref, eq_only = cp_reference(problem, x0, its, plot)
            where = f"cp_batch seed {seed} case {case} instance {k} of {batch} (n {x_ref.size}, {its} iterations, cadence {plot})"
            layer = _cp_single_agrees(problem, x0, its, x_ref)
            _require(np.array_equal(x[k], x_ref), where + ": the returned x differs", layer)
            _compare_reports(rec, k, ref, where, layer, vineq=not eq_only)
            if eq_only:
                _require(all(v[k] == 0 for v in rec.vineq), where + ": a violated inequality without inequality rows")
            _require(np.array_equal(xs[k], x_ref), where + ": x of the state differs", layer)
            _require(np.array_equal(ys[k], y_ref), where + ": y differs", layer)
            counts["instances"] += 1
            counts["reports"] += len(ref.it)
            counts["equalities_only"] += eq_only
        counts["batches"] += 1
    return counts


CP_MANY_SETTINGS = (("default", None, None), ("lds", "lds", None), ("global", "global", None), ("kmax1", None, 1))


def run_cp_many(cases, seed):
    """``chambolle_pock_ppd_many`` and ``CPManyState``: every LP of every list against the oracle, with the form chosen by the
    library, forced to ``lds`` and to ``global``, and with one iteration per launch.  Returns counts."""
    from pysparselp_amd import CPManyState, chambolle_pock_ppd_many
    from pysparselp_amd.ChambollePockPPD import _many_problem

    counts = dict(lists=0, lps=0, runs=0, equalities_only=0, longest=0)
    for case, (lps, its, plot) in enumerate(cp_many_cases(cases, seed)):
        problems = [of_instance(lp, 0)[0] for lp in lps]
        x0 = [lp["x0"] for lp in lps]
        refs = {}
        for k, lp in enumerate(lps):   # a cycled list repeats its LPs: one reference each
            if id(lp) not in refs:
                refs[id(lp)] = cp_reference(problems[k], x0[k], its, plot)
        for name, form, kmax in CP_MANY_SETTINGS:
            with environment(SLP_CP_MANY_FORM=form, SLP_CP_MANY_KMAX=kmax):
                rec = _Reports()
                xs, _ = chambolle_pock_ppd_many(problems, x0=x0, nb_max_iter=its, nb_iter_plot=plot, callback_func=rec)
                state = CPManyState([_many_problem(k, p) for k, p in enumerate(problems)], x0)
                try:
                    forms = [state.form(k) for k in range(state.count)]
                    sx, sy = _state_at_last_report(state, its)
                finally:
                    state.close()
            _require(form is None or set(forms) == {form}, f"cp_many seed {seed} case {case}: forms {set(forms)} under SLP_CP_MANY_FORM={form}")
            for k, lp in enumerate(lps):
                ref, x_ref, y_ref, eq_only = refs[id(lp)]
                where = (f"cp_many seed {seed} case {case} LP {k} of {len(lps)} (n {x_ref.size}, {its} iterations, cadence {plot}), "
                         f"setting {name}, form {forms[k]}")
                layer = _cp_single_agrees(problems[k], x0[k], its, x_ref)
                _require(np.array_equal(xs[k], x_ref), where + ": the returned x differs", layer)
                _compare_reports(rec, k, ref, where, layer, vineq=not eq_only)
                if eq_only:
                    _require(all(v[k] == 0 for v in rec.vineq), where + ": a violated inequality without inequality rows")
                _require(np.array_equal(sx[k], x_ref), where + ": x of the state differs", layer)
                _require(np.array_equal(sy[k], y_ref), where + ": y differs", layer)
            counts["runs"] += 1
        counts["lists"] += 1
        counts["lps"] += len(refs)
        counts["equalities_only"] += sum(r[3] for r in refs.values())
        counts["longest"] = max(counts["longest"], len(lps))
    return counts


# ---- ADMM ------------------------------------------------------------------------------------------------------------------------------

def admm_reference(problem, x0, its, plot):
    """``oracle.lp_admm`` on one LP: ``(reports, x, lambda as the report of iteration its sees it)``."""
    from oracle import oracle

    rec, last = _Reports(), {}

    def hook(i, x, x_all, lambda_eq):
        if i == its:
            last["lam"], last["x"] = lambda_eq.copy(), x.copy()

    x = oracle.lp_admm(*problem, x0=x0, nb_iter=its, nb_iter_plot=plot, callback_func=rec, iterate_hook=hook)
    assert np.array_equal(x, last["x"])
    return rec, x, last["lam"]


def _admm_single_agrees(problem, x0, its, x_ref):
    def layer():
        from pysparselp_amd import ORDER_SEQUENTIAL
        from pysparselp_amd.ADMM import lp_admm

        x = lp_admm(*problem, x0=x0, nb_iter=its, nb_iter_plot=10 ** 9, order=ORDER_SEQUENTIAL)
        return "lp_admm in ORDER_SEQUENTIAL on this LP alone " + ("AGREES" if np.array_equal(x, x_ref) else "DISAGREES") + " with the oracle"
    return layer


def run_admm_batch(cases, seed):
    """``lp_admm_batch`` and ``ADMMBatchState`` in both forms of the iteration: every instance against the oracle.  Returns counts."""
    from pysparselp_amd import ADMMBatchState, lp_admm_batch

    counts = dict(batches=0, instances=0, reports=0)
    for case, (args, its, plot) in enumerate(admm_batch_cases(cases, seed)):
        batch, n = args["c"].shape
        refs = [admm_reference(*of_instance(args, k), its, plot) for k in range(batch)]
        for form in ("tile", "levels"):
            with environment(SLP_ADMM_BATCH_FORM=form):
                rec = _Reports()
                x = lp_admm_batch(args["c"], args["a_eq"], args["beq"], args["a_ineq"], args["b_lower"], args["b_upper"], args["lb"],
                                  args["ub"], x0=args["x0"], nb_iter=its, nb_iter_plot=plot, callback_func=rec)
                state = ADMMBatchState(args["c"], args["a_eq"], args["beq"], args["a_ineq"], args["b_lower"], args["b_upper"], args["lb"],
                                       args["ub"], args["x0"])
                try:
                    _require(state.form() == form, f"admm_batch seed {seed} case {case}: form {state.form()} under {form}")
                    for p in _pieces(its):
                        state.iterate(p)
                    state.sweep_step()
                    xs, lam = state.x(n), state.lam()
                finally:
                    state.close()
            for k in range(batch):
                ref, x_ref, lam_ref = refs[k]
                problem, x0 = of_instance(args, k)
                where = f"admm_batch seed {seed} case {case} instance {k} of {batch} (n {n}, {its} iterations, cadence {plot}), form {form}"
                layer = _admm_single_agrees(problem, x0, its, x_ref)
                _require(np.array_equal(x[k], x_ref), where + ": the returned x differs", layer)
                _compare_reports(rec, k, ref, where, layer)
                _require(np.array_equal(xs[k], x_ref), where + ": x of the state differs", layer)
                _require(np.array_equal(lam[k], lam_ref), where + ": lambda differs", layer)
        counts["batches"] += 1
        counts["instances"] += batch
        counts["reports"] += sum(len(r[0].it) for r in refs)
    return counts


ADMM_MANY_SETTINGS = (("default", None, None), ("lds", "lds", None), ("global", "global", None), ("kmax1", None, 1))


def run_admm_many(cases, seed):
    """``lp_admm_many`` and ``ADMMManyState``: every LP of every list against the oracle at every report and at the end, with the
    form chosen by the library, forced to ``lds`` and to ``global``, and with one iteration per launch.  Returns counts."""
    from pysparselp_amd import ADMMManyState, lp_admm_many
    from pysparselp_amd.ADMM import _admm_many_problem, _admm_many_starts

    counts = dict(lists=0, lps=0, runs=0, longest=0)
    for case, (lps, its, plot) in enumerate(admm_many_cases(cases, seed)):
        problems = [of_instance(lp, 0)[0] for lp in lps]
        x0 = [lp["x0"] for lp in lps]
        refs = {}
        for k, lp in enumerate(lps):   # a cycled list repeats its LPs: one reference each
            if id(lp) not in refs:
                refs[id(lp)] = admm_reference(problems[k], x0[k], its, plot)
        for name, form, kmax in ADMM_MANY_SETTINGS:
            with environment(SLP_ADMM_MANY_FORM=form, SLP_ADMM_MANY_KMAX=kmax):
                rec = _Reports()
                xs = lp_admm_many(problems, x0=x0, nb_iter=its, nb_iter_plot=plot, callback_func=rec)
                checked = [_admm_many_problem(k, p) for k, p in enumerate(problems)]
                state = ADMMManyState(checked, _admm_many_starts(x0, checked))
                try:
                    forms = [state.form(k) for k in range(state.count)]
                    for p in _pieces(its):
                        state.iterate(p)
                    state.sweep_step()
                    sx, lam = state.x(), state.lam()
                finally:
                    state.close()
            _require(form is None or set(forms) == {form}, f"admm_many seed {seed} case {case}: forms {set(forms)} under SLP_ADMM_MANY_FORM={form}")
            for k, lp in enumerate(lps):
                ref, x_ref, lam_ref = refs[id(lp)]
                where = (f"admm_many seed {seed} case {case} LP {k} of {len(lps)} (n {x_ref.size}, {its} iterations, cadence {plot}), "
                         f"setting {name}, form {forms[k]}")
                layer = _admm_single_agrees(problems[k], x0[k], its, x_ref)
                _require(np.array_equal(xs[k], x_ref), where + ": the returned x differs", layer)
                _compare_reports(rec, k, ref, where, layer)
                _require(np.array_equal(sx[k], x_ref), where + ": x of the state differs", layer)
                _require(np.array_equal(lam[k], lam_ref), where + ": lambda differs", layer)
            counts["runs"] += 1
        counts["lists"] += 1
        counts["lps"] += len(refs)
        counts["longest"] = max(counts["longest"], len(lps))
    return counts


# ---- the per-LP stopping test of the two list solvers --------------------------------------------------------------------------------

class _StopReports(_Reports):
    """Also keeps the ``info`` the ``_until`` driver sets as an attribute of its callback, as it is at every call (copies)."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __call__(self, *report):
        super().__call__(*report)
        self.seen.append({name: np.array(values, copy=True) for name, values in self.info.items()})


def _stop_where(case_no, seed, case, setting, forms, width=None):
    """``where(k, run)``: the head of every message about LP ``k`` of the list (instance ``k`` of the batch, run with tiles of
    ``width`` instances) in the run ``run``."""
    def where(k, run):
        n = case.problems[k][0].size
        start = "cold" if case.x0[k] is None else "warm"
        who = f"{case.family}_many_stop seed {seed} case {case_no} LP {k} of {len(case.lps)}"
        if width is not None:
            who = f"admm_batch_stop seed {seed} case {case_no} instance {k} of B = {len(case.lps)}, tile width {width}"
        return (f"{who} (n {n}, {start} start, {case.total} iterations), "
                f"setting {setting}, form {forms[k]}, every {case.every}, tolerances {case.tol!r} (LP {case.k_star} at iteration {case.t_star}), {run}")
    return where


def _stop_layer(case, k, count):
    """Does the single solver agree with the oracle on LP ``k`` after ``count`` iterations?"""
    ref = case.ref(k)
    n = case.problems[k][0].size
    if case.family == "cp":
        return _cp_single_agrees(case.problems[k], case.x0[k], count, ref.xs[count])
    return _admm_single_agrees(case.problems[k], case.x0[k], count - 1, ref.xs[count][:n])


STOP_NAMES = {"cp": ("iterations", "stopped", "step"), "admm": ("iterations", "stopped", "residual", "step")}


def _compare_stop(case, want, got, iterates, where, run, dtypes=False):
    """``got`` (the columns of ``stop_state``, or of the driver's ``info``) against the restatement's ``want`` with
    ``np.array_equal``, and -- unless ``iterates`` is None -- every LP's primal and dual iterate against the oracle's at that LP's
    own count, bit for bit.  A NaN equals a NaN, so a column differs wherever the restatement holds none and the device one.
    ``dtypes``: the columns also have the restatement's types."""
    for name, g, w in zip(STOP_NAMES[case.family], got, want):
        _require(not dtypes or g.dtype == w.dtype, where(0, run) + f": {name} has type {g.dtype}, the restatement's has {w.dtype}")
        if not np.array_equal(g, w, equal_nan=(name not in ("iterations", "stopped"))):
            k = next(k for k in range(len(w)) if not np.array_equal(g[k], w[k], equal_nan=True))
            count = max(1, int(min(got[0][k], want[0][k], case.total)))
            _require(False, where(k, run) + f": {name} {g[k]!r}, the restatement gives {w[k]!r}", _stop_layer(case, k, count))
    if iterates is None:
        return
    for k in range(len(case.lps)):
        ref, count = case.ref(k), int(want[0][k])
        for name, g, r in (("x", iterates[0][k], ref.xs[count]), ("y" if case.family == "cp" else "lambda", iterates[1][k], ref.duals[count])):
            _require(np.array_equal(g, r), where(k, run) + f": {name} differs from the oracle's after {count} iterations", _stop_layer(case, k, count))


def _compare_stop_driver(case, want, xs, info, rec, where):
    """The ``_until`` driver: ``info`` is the restatement, ``xs[k]`` the oracle's ``x`` at each LP's count; at every callback a stopped
    LP has its final iterate and ``callback_func.info`` says so, a running one has the oracle's report (energies within
    ``ENERGY_TOL``).  The loop ends at the first report index at which every LP is stopped."""
    run = f"the driver with reports every {case.plot}"
    _compare_stop(case, want, tuple(info[name] for name in STOP_NAMES[case.family]), None, where, run)
    last = int(want[0].max()) if want[1].all() else case.total
    reports = [i for i in range(0, case.total, case.plot) if i < last]
    _require(rec.it == reports, where(0, run) + f": reports at {rec.it}, expected at {reports}")
    for k in range(len(case.lps)):
        ref, count = case.ref(k), int(want[0][k])
        n = case.problems[k][0].size
        layer = _stop_layer(case, k, count)
        x_final = ref.xs[count][:n]
        _require(np.array_equal(xs[k], x_final), where(k, run) + f": the returned x differs from the oracle's after {count} iterations", layer)
        for i, it in enumerate(reports):
            at = where(k, run) + f", report at iteration {it}"
            stopped = bool(want[1][k]) and count <= it
            _require(bool(rec.seen[i]["stopped"][k]) == stopped, at + f": info['stopped'] is {rec.seen[i]['stopped'][k]}, the restatement stops it at {count}")
            _require(int(rec.seen[i]["iterations"][k]) == (count if stopped else it), at + f": info['iterations'] is {rec.seen[i]['iterations'][k]}")
            if stopped:
                _require(np.array_equal(rec.x[i][k], x_final), at + ": a stopped LP's x is not its final iterate", layer)
                if case.family == "admm":   # the report on the frozen state: its residual is the recorded one
                    _require(rec.veq[i][k] == want[2][k], at + f": max violated equality {rec.veq[i][k]!r}, recorded residual {want[2][k]!r}", layer)
                continue
            _require(ref.reports.it[i] == it, at + f": the oracle reports at {ref.reports.it[i]}")
            _require(np.array_equal(rec.x[i][k], ref.reports.x[i]), at + ": x differs", layer)
            _require(rec.veq[i][k] == ref.reports.veq[i], at + f": max violated equality {rec.veq[i][k]!r} != {ref.reports.veq[i]!r}", layer)
            if ref.eq_only:
                _require(rec.vineq[i][k] == 0, at + ": a violated inequality without inequality rows")
            else:
                _require(rec.vineq[i][k] == ref.reports.vineq[i], at + f": max violated inequality {rec.vineq[i][k]!r} != {ref.reports.vineq[i]!r}", layer)
            for name, g, r in (("energy1", rec.e1[i][k], ref.reports.e1[i]), ("energy2", rec.e2[i][k], ref.reports.e2[i])):
                _require(np.allclose(g, r, equal_nan=True, **ENERGY_TOL), at + f": {name} {g!r} != {r!r}", layer)


def _run_many_stop(family, cases, seed):
    """Both ``run_*_many_stop`` and, with ``family == "admm_batch"``, ``run_admm_batch_stop``: see there."""
    batched = family == "admm_batch"

    def forms_of(state):   # a batch has one form
        return [state.form()] * state.batch if batched else [state.form(k) for k in range(state.count)]

    if family == "cp":
        from pysparselp_amd import CPManyState, chambolle_pock_ppd_many_until
        from pysparselp_amd.ChambollePockPPD import _many_problem

        settings, switches = (lambda case: CP_MANY_SETTINGS), ("SLP_CP_MANY_FORM", "SLP_CP_MANY_KMAX")
        stop_cases = cp_stop_cases(cases, seed)

        def create(case):
            return CPManyState([_many_problem(k, p) for k, p in enumerate(case.problems)], case.x0)

        def halves(state):
            state.primal_step()
            state.dual_step()

        def iterates(state):
            return state.x(), state.y()

        def driver(case, rec):
            xs, _, info = chambolle_pock_ppd_many_until(case.problems, *case.tol, case.every, x0=case.x0, nb_max_iter=case.total, callback_func=rec,
                                                        nb_iter_plot=case.plot)
            return xs, info
    elif batched:
        from pysparselp_amd import ADMMBatchState, lp_admm_batch_until

        settings, switches = (lambda case: admm_batch_stop_settings(case.width)), ("SLP_ADMM_BATCH_FORM", "SLP_ADMM_BATCH_TILE")
        stop_cases = admm_batch_stop_cases(cases, seed)

        def blocks(case):
            a = case.args
            return a["c"], a["a_eq"], a["beq"], a["a_ineq"], a["b_lower"], a["b_upper"], a["lb"], a["ub"]

        def create(case):
            return ADMMBatchState(*blocks(case), case.args["x0"])

        def halves(state):
            state.sweep_step()
            state.multiplier_step()

        def iterates(state):
            return state.x(), state.lam()

        def driver(case, rec):   # nb_iter + 1 sweeps
            return lp_admm_batch_until(*blocks(case), *case.tol, case.every, x0=case.args["x0"], nb_iter=case.total - 1, callback_func=rec,
                                       nb_iter_plot=case.plot)
    else:
        from pysparselp_amd import ADMMManyState, lp_admm_many_until
        from pysparselp_amd.ADMM import _admm_many_problem, _admm_many_starts

        settings, switches = (lambda case: ADMM_MANY_SETTINGS), ("SLP_ADMM_MANY_FORM", "SLP_ADMM_MANY_KMAX")
        stop_cases = admm_stop_cases(cases, seed)

        def create(case):
            checked = [_admm_many_problem(k, p) for k, p in enumerate(case.problems)]
            return ADMMManyState(checked, _admm_many_starts(case.x0, checked))

        def halves(state):
            state.sweep_step()
            state.multiplier_step()

        def iterates(state):
            return state.x(full=True), state.lam()

        def driver(case, rec):   # nb_iter + 1 sweeps
            return lp_admm_many_until(case.problems, *case.tol, case.every, x0=case.x0, nb_iter=case.total - 1, callback_func=rec,
                                      nb_iter_plot=case.plot)

    def armed_run(case, unarmed, split_at=None, calls=()):
        """A fresh state: ``unarmed`` iterations, ``set_stop``, the rest up to ``total`` (the iteration ``split_at`` in its two halves;
        a further ``set_stop(*arguments)`` once ``at`` iterations are complete for each ``(at, arguments)`` of ``calls``).  Returns
        ``(forms, stop_state, iterates, column 1 of the report, [(at, stop_state before the call, after it)])``."""
        state = create(case)
        try:
            forms = forms_of(state)
            for p in _pieces(unarmed):
                state.iterate(p)
            state.set_stop(*case.tol, case.every)
            done, marks = unarmed, []
            if split_at is not None:
                for p in _pieces(split_at - 1 - done):
                    state.iterate(p)
                halves(state)
                done = split_at
            for at, arguments in calls:
                for p in _pieces(at - done):
                    state.iterate(p)
                done, before = at, state.stop_state()
                state.set_stop(*arguments)
                marks.append((at, before, state.stop_state()))
            for p in _pieces(case.total - done):
                state.iterate(p)
            return forms, state.stop_state(), iterates(state), (None if family == "cp" else state.report()[:, 1]), marks
        finally:
            state.close()

    counts = dict(lists=0, entries=0, lps=0, runs=0, stopped=0, running=0, longest=0, mixed_tiles=0, dead_tiles=0)
    for case_no, case in enumerate(stop_cases):
        want = case.want()
        for name, form, kmax in settings(case):
            with environment(**dict(zip(switches, (form, kmax)))):
                forms, got, its, residual, _ = armed_run(case, 0)   # (a) armed from creation
                _require(form is None or set(forms) == {form}, f"{'admm_batch' if batched else family + '_many'}_stop seed {seed} case {case_no}: forms {set(forms)} under {switches[0]}={form}")
                width = (kmax or admm_batch_width(forms[0], len(case.lps))) if batched else None
                where = _stop_where(case_no, seed, case, name, forms, width)
                _compare_stop(case, want, got, its, where, "armed from creation", dtypes=batched)
                if family != "cp":
                    for k in np.nonzero(want[1])[0]:
                        _require(residual[k] == want[2][k], where(k, "armed from creation") + f": the report's residual {residual[k]!r} of a stopped LP, "
                                 f"recorded {want[2][k]!r}", _stop_layer(case, k, int(want[0][k])))
                if batched:
                    mixed, dead = stop_tiles(want, width, case.every)
                    counts["mixed_tiles"] += mixed
                    counts["dead_tiles"] += dead
                if name == "default":
                    _, got, its, _, _ = armed_run(case, case.after)   # (b) armed in mid-life
                    _compare_stop(case, case.want(after=case.after), got, its, where, f"armed after {case.after} iterations", dtypes=batched)
                    _, got, its, _, _ = armed_run(case, 0, split_at=case.t_star)   # (c) the iteration t_star in its two halves
                    _compare_stop(case, want, got, its, where, f"iteration {case.t_star} in two halves", dtypes=batched)
                    if batched:   # (d) armed again with halved tolerances, then off: the flags and the last evaluated numbers stay
                        schedule = case.schedule()
                        run = f"armed again at {case.rearm} with halved tolerances, off at {case.off}"
                        _, got, its, _, marks = armed_run(case, 0, calls=[(case.rearm, schedule[1][1:]), (case.off, (None, None))])
                        for i, (at, before, after) in enumerate(marks):
                            _compare_stop(case, case.want(schedule=schedule[:i + 1], total=at), before, None, where, run + f", after {at} iterations", dtypes=True)
                            _compare_stop(case, before, after, None, where, run + f", after the call of set_stop at {at}", dtypes=True)
                        _compare_stop(case, case.want(schedule=schedule), got, its, where, run, dtypes=True)
                    rec = _StopReports()   # the driver
                    xs, info = driver(case, rec)
                    _compare_stop_driver(case, want, xs, info, rec, where)
            counts["runs"] += 1
        counts["lists"] += 1
        counts["entries"] += len(case.lps)
        counts["lps"] += case.distinct()
        counts["stopped"] += int(want[1].sum())
        counts["running"] += int((~want[1]).sum())
        counts["longest"] = max(counts["longest"], len(case.lps))
    if batched:
        return dict(batches=counts["lists"], instances=counts["entries"], distinct=counts["lps"],
                    **{name: counts[name] for name in ("runs", "stopped", "running", "longest", "mixed_tiles", "dead_tiles")})
    return {name: counts[name] for name in ("lists", "lps", "runs", "stopped", "running", "longest")}


def run_cp_many_stop(cases, seed):
    """``CPManyState.set_stop`` / ``stop_state`` and ``chambolle_pock_ppd_many_until`` on the lists of ``run_cp_many``, each with a
    stopping test whose tolerance is the reference step of one of its LPs at a check iteration (``<=`` decides by equality), 20
    iterations longer.  Under the four settings of ``run_cp_many``, armed from creation: ``stop_state`` against the restatement
    (tests/cp_stop_cpu.py) and every LP's ``x`` and ``y`` against the oracle's iterate at that LP's own count.  With the library's own
    choice also: armed in mid-life, the chosen iteration in its two halves, and the driver with its callbacks.  Returns counts."""
    return _run_many_stop("cp", cases, seed)


def run_admm_many_stop(cases, seed):
    """``ADMMManyState.set_stop`` / ``stop_state`` and ``lp_admm_many_until`` on the lists of ``run_admm_many``: as
    ``run_cp_many_stop``, with the two tolerances the reference residual and step of one LP at a check iteration
    (tests/admm_stop_cpu.py), ``x`` over all columns of the standard form, ``lambda``, and a stopped LP's report against its
    recorded residual.  Returns counts."""
    return _run_many_stop("admm", cases, seed)


def run_admm_batch_stop(cases, seed):
    """``ADMMBatchState.set_stop`` / ``stop_state`` and ``lp_admm_batch_until`` on the batches of ``admm_batch_stop_cases``, as
    ``run_admm_many_stop`` does for the lists; no instance is left out.  Under six settings -- the library's own choice, the tile and
    the levels form with the case's drawn tile width and with width 64, the levels form with width 1 -- armed from creation:
    ``stop_state`` with ``np.array_equal`` and its types against tests/admm_batch_stop_cpu.py, ``x`` over all columns of the standard form and
    ``lambda`` of every instance against the oracle's at that instance's own count, bit for bit, a stopped instance's report against
    its recorded residual.  With the library's own choice also: armed in mid-life; the drawn iteration in its two halves; armed
    again at a check before it with both tolerances halved and turned off later (``stop_state`` before and after either call and
    at the end); the driver with its callbacks.  Returns counts; ``mixed_tiles`` and ``dead_tiles`` (``stop_tiles``) are summed
    over the runs armed from creation."""
    return _run_many_stop("admm_batch", cases, seed)


# ---- the certified stopping test of the Chambolle-Pock list solver and of the batched one ------------------------------------------------

GAP_NAMES = ("iterations", "stopped", "primal", "lower_bound", "violation")


def _gap_where(name, case_no, seed, case, setting, forms):
    """``where(k, run)``: the head of every message about entry ``k`` of the case in the run ``run``."""
    def where(k, run):
        ref = case.entries[k]
        what = f"LP {k} of {len(case.entries)}" if case.family == "many" else f"instance {k} of {len(case.entries)}"
        return (f"{name} seed {seed} case {case_no} {what} (n {ref.n}, {'warm' if ref.warm else 'cold'} start, {'boxed' if ref.boxed else 'as drawn'}, "
                f"{case.total} iterations), setting {setting}, form {forms[k]}, every {case.every}, tolerances {case.tol!r} "
                f"(entry {case.k_star} at iteration {case.t_star}), {run}")
    return where


def _gap_layer(case, k, count):
    """Does the single solver agree with the oracle on entry ``k`` after ``count`` iterations?"""
    ref = case.entries[k]
    count = max(1, min(int(count), case.total))
    return _cp_single_agrees(ref.problem, ref.x0, count, ref.xs[count])


def _compare_gap(case, want, keep, got, iterates, where, run):
    """``got`` (the columns of ``gap_state``, or of the driver's ``info``) against the restatement's ``want``: iterations and flags
    with ``np.array_equal`` on the kept entries, and where both sides evaluated the same check last the violation exactly, primal
    and bound within ``ENERGY_TOL``.  Unless ``iterates`` is None every entry's ``x`` and ``y`` against the oracle's at that entry's
    own count (a left-out entry: at the device's count), bit for bit.  Returns the counts the iterates were compared at."""
    same = keep | (got[0] == want[0])
    for name, g, w in zip(GAP_NAMES, got, want):
        with np.errstate(invalid="ignore"):
            if name in ("iterations", "stopped"):
                bad = keep & (g != w)
            elif name == "violation":
                bad = same & ~((g == w) | (np.isnan(g) & np.isnan(w)))
            else:
                bad = same & ~np.isclose(g, w, equal_nan=True, **ENERGY_TOL)
        if bad.any():
            k = int(np.nonzero(bad)[0][0])
            _require(False, where(k, run) + f": {name} {g[k]!r}, the restatement gives {w[k]!r}", _gap_layer(case, k, min(got[0][k], want[0][k])))
    counts = np.where(keep, want[0], got[0])
    _require(bool(np.all((counts >= 0) & (counts <= case.total))), where(0, run) + f": iteration counts {got[0]} outside the run")
    if iterates is not None:
        for k, ref in enumerate(case.entries):
            count = int(counts[k])
            for name, g, r in (("x", iterates[0][k], ref.xs[count]), ("y", iterates[1][k], ref.ys[count])):
                _require(np.array_equal(g, r), where(k, run) + f": {name} differs from the oracle's after {count} iterations", _gap_layer(case, k, count))
    return counts


def _compare_gap_driver(case, want, keep, xs, info, rec, where):
    """The ``_certified`` driver: ``info`` is the restatement, ``xs[k]`` the oracle's ``x`` at each entry's count; at every callback a
    stopped entry has its final iterate and ``callback_func.info`` says so, a running one has the oracle's report (energies within
    ``ENERGY_TOL``).  The loop ends at the first report index at which every entry is stopped.  A left-out entry is followed at
    the device's own count."""
    run = f"the driver with reports every {case.plot}"
    got = tuple(info[name] for name in GAP_NAMES)
    counts = _compare_gap(case, want, keep, got, None, where, run)
    stops = np.where(keep, want[1], got[1])
    last = int(counts.max()) if stops.all() else case.total
    reports = [i for i in range(0, case.total, case.plot) if i < last]
    _require(rec.it == reports, where(0, run) + f": reports at {rec.it}, expected at {reports}")
    for k, ref in enumerate(case.entries):
        count = int(counts[k])
        layer = _gap_layer(case, k, count)
        _require(np.array_equal(xs[k], ref.xs[count]), where(k, run) + f": the returned x differs from the oracle's after {count} iterations", layer)
        for i, it in enumerate(reports):
            at = where(k, run) + f", report at iteration {it}"
            stopped = bool(stops[k]) and count <= it
            _require(bool(rec.seen[i]["stopped"][k]) == stopped, at + f": info['stopped'] is {rec.seen[i]['stopped'][k]}, it stops at {count}")
            _require(int(rec.seen[i]["iterations"][k]) == (count if stopped else it), at + f": info['iterations'] is {rec.seen[i]['iterations'][k]}")
            if stopped:
                _require(np.array_equal(rec.x[i][k], ref.xs[count]), at + ": a stopped entry's x is not its final iterate", layer)
                continue
            _require(ref.reports.it[i] == it, at + f": the oracle reports at {ref.reports.it[i]}")
            _require(np.array_equal(rec.x[i][k], ref.reports.x[i]), at + ": x differs", layer)
            _require(rec.veq[i][k] == ref.reports.veq[i], at + f": max violated equality {rec.veq[i][k]!r} != {ref.reports.veq[i]!r}", layer)
            if ref.eq_only:
                _require(rec.vineq[i][k] == 0, at + ": a violated inequality without inequality rows")
            else:
                _require(rec.vineq[i][k] == ref.reports.vineq[i], at + f": max violated inequality {rec.vineq[i][k]!r} != {ref.reports.vineq[i]!r}", layer)
            for name, g, r in (("energy1", rec.e1[i][k], ref.reports.e1[i]), ("energy2", rec.e2[i][k], ref.reports.e2[i])):
                _require(np.allclose(g, r, equal_nan=True, **ENERGY_TOL), at + f": {name} {g!r} != {r!r}", layer)


def _check_gap_bounds(counts, case, keep, got, iterates, where):
    """The final record of every entry of the run armed from creation, taken where the last check was the last iteration (so
    that the device's ``y`` is the record's): the device's bound against ``cp_gap_cpu.exact_bound`` on the device's own ``y``, and
    bound and primal against HiGHS."""
    run, cache = "the final record", {}
    for k, ref in enumerate(case.entries):
        t, stopped, primal, bound, violation = (col[k] for col in got)
        x, y = iterates[0][k], iterates[1][k]
        key = (id(ref), int(t), float(bound), y.tobytes())
        if key not in cache:   # a cycled list repeats its LPs
            with np.errstate(invalid="ignore", over="ignore"):
                cache[key] = gap_exact_bound(ref, y), ref.restated.at(x, y).band
        exact, band = cache[key]
        kind = gap_bound_kind(bound, exact, band)
        layer = _gap_layer(case, k, t)
        _require(kind is not None, where(k, run) + f" after {t} iterations: lower bound {bound!r}, exactly {exact!r} on the device's y (band {band!r})", layer)
        counts["bounds_checked"] += 1
        counts["rounded_to_zero"] += bool(keep[k]) and kind == "rounded to zero"
        res = ref.highs()
        if res.status == 3:
            _require(bound == -np.inf and not stopped, where(k, run) + f": HiGHS calls the LP unbounded; lower bound {bound!r}, stopped {stopped}", layer)
            counts["unbounded"] += 1
            continue
        if res.status == 2:   # a perturbed right-hand side (``batch_of``) can leave no feasible point: every bound is valid then
            counts["infeasible"] += 1
            continue
        _require(res.status == 0, where(k, run) + f": linprog status {res.status} ({res.message})")
        slack = gap_highs_slack(band, res.fun)
        if np.isfinite(bound):
            _require(bound <= res.fun + slack, where(k, run) + f": the lower bound {bound!r} exceeds the optimum {res.fun!r} by more than {slack!r}", layer)
            counts["bounds_below_optimum"] += 1
        if stopped and violation == 0.0:
            _require(primal >= res.fun - slack, where(k, run) + f": primal {primal!r} of a feasible iterate lies below the optimum {res.fun!r} by more "
                     f"than {slack!r}", layer)
            counts["primals_above_optimum"] += 1


def _run_gap(name, cases, seed, stop_cases, settings, switches, create, rows, driver, split):
    """Both certificate runs: see ``run_cp_many_gap`` and ``run_cp_batch_gap``.  ``create(case)``: a fresh state; ``rows(state)``:
    ``(forms, x, y)`` with one row per entry; ``driver(case, rec)``: ``(xs, info)``; ``split``: also the iteration ``t_star`` in
    its two halves."""
    def armed_run(case, unarmed, split_at=None, pause_at=None):
        """A fresh state: ``unarmed`` iterations, ``set_stop_gap``, the rest up to ``total`` (the iteration ``split_at`` in its two
        halves).  Returns ``(forms, gap_state, stop_state()[:2] or None, (x, y), the same three after pause_at iterations)``."""
        state = create(case)
        try:
            for p in _pieces(unarmed):
                state.iterate(p)
            state.set_stop_gap(*case.tol, case.every)
            done, paused = unarmed, None
            if split_at is not None:
                for p in _pieces(split_at - 1 - done):
                    state.iterate(p)
                state.primal_step()
                state.dual_step()
                done = split_at
            if pause_at is not None and pause_at < case.total:
                for p in _pieces(pause_at - done):
                    state.iterate(p)
                done = pause_at
                paused = state.gap_state(), rows(state)[1:]
            for p in _pieces(case.total - done):
                state.iterate(p)
            forms, x, y = rows(state)
            got = state.gap_state()
            return forms, got, (state.stop_state()[:2] if hasattr(state, "stop_state") else None), (x, y), paused or (got, (x, y))
        finally:
            state.close()

    left_out = sum(int((~case.keep()).sum()) for case in stop_cases)
    entries = sum(len(case.entries) for case in stop_cases)
    _require(left_out <= GAP_LEFT_OUT * entries, f"{name} seed {seed}: {left_out} of {entries} entries have an undecidable check, more than 5 %")
    counts = dict(lists=0, lps=0, runs=0, stopped=0, running=0, left_out=0, longest=0, bounds_checked=0, bounds_below_optimum=0,
                  primals_above_optimum=0, unbounded=0, infeasible=0, rounded_to_zero=0)
    for case_no, case in enumerate(stop_cases):
        want, keep = case.want(), case.keep()
        for setting, form, kmax in settings:
            with environment(**dict(zip(switches, (form, kmax)))):
                default = setting == "default"
                last_check = case.total - case.total % case.every
                forms, got, flags, its, paused = armed_run(case, 0, pause_at=last_check if default else None)   # (a) armed from creation
                where = _gap_where(name, case_no, seed, case, setting, forms)
                _require(form is None or set(forms) == {form}, f"{name} seed {seed} case {case_no}: forms {set(forms)} under {switches[0]}={form}")
                _compare_gap(case, want, keep, got, its, where, "armed from creation")
                if flags is not None:
                    _require(np.array_equal(flags[0], got[0]) and np.array_equal(flags[1], got[1]), where(0, "armed from creation") +
                             f": stop_state gives {flags[0]}, {flags[1]}, gap_state {got[0]}, {got[1]}")
                if default:
                    _check_gap_bounds(counts, case, keep, *paused, where)
                    late, keep_late = case.want(after=case.after), case.keep(case.after)   # (b) armed in mid-life
                    _, got, _, its, _ = armed_run(case, case.after)
                    _compare_gap(case, late, keep_late, got, its, where, f"armed after {case.after} iterations")
                    if split:   # (c) the iteration t_star in its two halves
                        _, got, _, its, _ = armed_run(case, 0, split_at=case.t_star)
                        _compare_gap(case, want, keep, got, its, where, f"iteration {case.t_star} in two halves")
                    rec = _StopReports()   # (d) the driver
                    xs, info = driver(case, rec)
                    _compare_gap_driver(case, want, keep, xs, info, rec, where)
            counts["runs"] += 1
        counts["lists"] += 1
        counts["lps"] += len(case.distinct())
        counts["stopped"] += int((want[1] & keep).sum())
        counts["running"] += int((~want[1] & keep).sum())
        counts["left_out"] += int((~keep).sum())
        counts["longest"] = max(counts["longest"], len(case.entries))
    return counts


def run_cp_many_gap(cases, seed):
    """``CPManyState.set_stop_gap`` / ``gap_state`` and ``chambolle_pock_ppd_many_certified`` on the lists of ``cp_gap_cases`` (three
    quarters of the LPs keep their finite bounds, so that the certificate's sums are finite at the sizes the lists are drawn for).
    The tolerances are the violation and the relative gap of one LP at a check iteration (``GapCase``).  Under the four settings of
    ``run_cp_many``, armed from creation: ``gap_state`` against the restatement (tests/cp_gap_cpu.py) -- iterations and flags with
    ``np.array_equal`` for every LP all of whose checks are decidable, the violation exactly, primal and bound within ``ENERGY_TOL``
    -- ``stop_state`` in agreement with it, and every LP's ``x`` and ``y`` against the oracle's at that LP's own count.  With the
    library's own choice also: armed in mid-life, the drawn iteration in its two halves, the driver with its callbacks, and at the
    last check of the run every LP's recorded bound against ``cp_gap_cpu.exact_bound`` on the device's own ``y`` (within the band
    of rounding; a finite bound over an exact ``-inf`` is counted) and against HiGHS: no finite bound above the optimum, no
    feasible stopped iterate below it, ``-inf`` and running where the LP is unbounded.  Returns counts."""
    from pysparselp_amd import CPManyState, chambolle_pock_ppd_many_certified
    from pysparselp_amd.ChambollePockPPD import _many_problem

    def create(case):
        return CPManyState([_many_problem(k, ref.problem) for k, ref in enumerate(case.entries)], [ref.x0 for ref in case.entries])

    def rows(state):
        return [state.form(k) for k in range(state.count)], state.x(), state.y()

    def driver(case, rec):
        xs, _, info = chambolle_pock_ppd_many_certified([ref.problem for ref in case.entries], *case.tol, case.every, x0=[ref.x0 for ref in case.entries],
                                                        nb_max_iter=case.total, callback_func=rec, nb_iter_plot=case.plot)
        return xs, info

    stop_cases = cp_gap_cases(cases, seed)
    counts = _run_gap("cp_many_gap", cases, seed, stop_cases, CP_MANY_SETTINGS, ("SLP_CP_MANY_FORM", "SLP_CP_MANY_KMAX"), create, rows, driver, True)
    want = gap_statistics(stop_cases)["rounded_to_zero"]
    _require(counts["rounded_to_zero"] == want, f"cp_many_gap seed {seed}: {counts['rounded_to_zero']} final records have a finite bound over an exact "
             f"-inf, the restatement has {want}")
    return counts


def run_cp_batch_gap(cases, seed):
    """``CPBatchState.set_stop_gap`` / ``gap_state`` and ``chambolle_pock_ppd_batch_certified`` on the batches of
    ``cp_batch_gap_cases``: as ``run_cp_many_gap`` with one setting -- armed from creation, armed in mid-life, the driver, the
    recorded bounds against ``cp_gap_cpu.exact_bound`` and HiGHS -- every instance's ``x`` and ``y`` against the oracle's at that
    instance's own count.  In the counts ``lists`` are batches and ``lps`` instances.  Returns counts."""
    from pysparselp_amd import CPBatchState, chambolle_pock_ppd_batch_certified
    from pysparselp_amd.ChambollePockPPD import one_sided_system_batch

    def create(case):
        a = case.args
        ineq, b_ineq = (None, None) if a["a_ineq"] is None else one_sided_system_batch(a["a_ineq"], a["b_lower"], a["b_upper"])
        return CPBatchState(a["c"], a["a_eq"], a["beq"], ineq, b_ineq, a["lb"], a["ub"], a["x0"], 1, 1)

    def rows(state):
        return ["batch"] * state.batch, state.x(), state.y()

    def driver(case, rec):
        a = case.args
        xs, _, info = chambolle_pock_ppd_batch_certified(a["c"], a["a_eq"], a["beq"], a["a_ineq"], a["b_lower"], a["b_upper"], a["lb"], a["ub"],
                                                         *case.tol, case.every, x0=a["x0"], nb_max_iter=case.total, callback_func=rec,
                                                         nb_iter_plot=case.plot)
        return xs, info

    stop_cases = cp_batch_gap_cases(cases, seed)
    counts = _run_gap("cp_batch_gap", cases, seed, stop_cases, (("default", None, None),), ("SLP_CP_MANY_FORM", "SLP_CP_MANY_KMAX"), create, rows, driver,
                      False)
    want = gap_statistics(stop_cases)["rounded_to_zero"]
    _require(counts["rounded_to_zero"] == want, f"cp_batch_gap seed {seed}: {counts['rounded_to_zero']} final records have a finite bound over an exact "
             f"-inf, the restatement has {want}")
    return counts


# ---- dual gradient ascent on the device -------------------------------------------------------------------------------------------------

class _LP:
    """The attributes ``dual_gradient_ascent_many`` reads."""

    def __init__(self, c, a_eq, b_eq, a_ineq, b_upper, lb, ub):
        self.costsvector, self.a_equalities, self.b_equalities = c, a_eq, b_eq
        self.a_inequalities, self.b_upper, self.b_lower = a_ineq, b_upper, None
        self.lower_bounds, self.upper_bounds = lb, ub


def _start(lp):
    """The reference's start (seed 0) for the LP's shape and the generator its tie draws continue."""
    m_eq, m_in = lp.rows
    rs = np.random.RandomState(0)
    y_eq = -rs.rand(m_eq)
    y_ineq = np.abs(rs.rand(m_in)) if lp.args[3] is not None else np.zeros(0)
    return np.concatenate((y_eq, y_ineq)), rs


def _rhs(lp):
    return np.concatenate((lp.args[2], lp.args[4] if lp.args[3] is not None else np.zeros(0)))


@contextlib.contextmanager
def single_state(lp, path):
    from pysparselp_amd.DualGradientAscent import DeviceDGA
    from pysparselp_amd.device import DeviceMatrix

    c, a_eq, _, a_ineq, _, lb, ub = lp.args
    y0, rs = _start(lp)
    mat = DeviceMatrix.from_blocks(a_eq, a_ineq, c.size)
    state = None
    try:
        state = DeviceDGA(mat, _rhs(lp), c, lb, ub, y0, m_eq=a_eq.shape[0], draws=rs.random_sample, path=path)
        _require(state.path() == path, f"{lp.name}: path {state.path()} under {path}")
        yield state
    finally:
        if state is not None:
            state.close()
        mat.close()


@contextlib.contextmanager
def batch_state(lps, path):
    """``DeviceDGABatch`` over LPs that share the matrix and the right-hand sides; ``path``: ``fused``, ``general-segmented`` or
    ``general-global``."""
    from pysparselp_amd.DualGradientAscent import DeviceDGABatch
    from pysparselp_amd.device import DeviceMatrix

    c, a_eq, _, a_ineq, _, _, _ = lps[0].args
    y0, rs = _start(lps[0])
    path, _, sort = path.partition("-")
    mat = DeviceMatrix.from_blocks(a_eq, a_ineq, c.size)
    state = None
    try:
        with environment(SLP_DGA_BATCH_SORT=sort or None):
            state = DeviceDGABatch(mat, _rhs(lps[0]), np.array([lp.args[0] for lp in lps]), np.array([lp.args[5] for lp in lps]),
                                   np.array([lp.args[6] for lp in lps]), y0, m_eq=a_eq.shape[0], draws=rs.random_sample, path=path)
        _require((state.path(), state.sort()) == (path, sort or None), f"{lps[0].name}: path {state.path()}, sort {state.sort()}")
        yield state
    finally:
        if state is not None:
            state.close()
        mat.close()


@contextlib.contextmanager
def many_state(lps, kmax=None):
    from pysparselp_amd.DualGradientAscent import DeviceDGAMany, _dga_many_lp, dga_many_start

    forms = [_dga_many_lp(k, _LP(*lp.args)) for k, lp in enumerate(lps)]
    y0s, offsets = dga_many_start(forms)
    with environment(SLP_DGA_MANY_KMAX=kmax):
        state = DeviceDGAMany(forms, y0s, offsets)
    try:
        yield state
    finally:
        state.close()


def _snapshot(state, single=False):
    """``(x, y_eq, y_ineq, draws, flags)``, each indexed by instance / LP (a single state: as a list of one)."""
    flags, draws, _, _ = state.status()
    y_eq, y_ineq = state.y()
    if single:
        return [state.x()], [y_eq], [y_ineq], [draws], [flags]
    return state.x(), y_eq, y_ineq, draws, flags


def _walk(state, stops, single=False):
    """``{stop: snapshot}`` after ``stop + 1`` iterations, the iterations split over calls of uneven size."""
    out, done = {}, 0
    for s in stops:
        for p in _pieces(s + 1 - done):
            state.iterate(p)
        done = s + 1
        out[s] = _snapshot(state, single)
    return out


def _instance_equals(snap, k, ref):
    """Which of x, y_eq, y_ineq, draws of instance ``k`` differ from ``ref = (x, y_eq, y_ineq, draws)``: a list of names."""
    x, y_eq, y_ineq, draws, _ = snap
    want_ineq = ref[2] if ref[2] is not None else np.zeros(0)
    pairs = (("x", x[k], ref[0]), ("y_eq", y_eq[k], ref[1]), ("y_ineq", y_ineq[k], want_ineq))
    return [name for name, g, r in pairs if not np.array_equal(g, r)] + ([] if int(draws[k]) == ref[3] else ["draws"])


def single_result(lp, path):
    """The single solver on the LP alone, cached per path: ``dict(snaps={stop: snapshot}, report)`` at the LP's stops and after
    all ``DGA_ITERS`` iterations."""
    if path not in lp.single:
        stops = sorted(set(lp.stops()) | set(DGA_STOPS))
        with single_state(lp, path) as state:
            snaps = _walk(state, stops, single=True)
            lp.single[path] = dict(snaps=snaps, report=state.report())
    return lp.single[path]


def _dga_single_agrees(lp, path):
    def layer():
        got = single_result(lp, path)
        bad = [s for s, ref in _references(lp) if got["snaps"][s][4][0] != 0 or _instance_equals(got["snaps"][s], 0, ref)]
        return f"DeviceDGA ({path}) on this LP alone " + ("AGREES with dga_cpu" if not bad else f"DISAGREES with dga_cpu at {bad}")
    return layer


def _references(lp):
    """``[(stop, (x, y_eq, y_ineq, draws))]``: the reference's order up to the horizon, the ``"device"`` order behind it."""
    return [(s, lp.states[s]) for s in lp.stops()] + [(s, lp.device_states[s]) for s in lp.late_stops()]


def _compare_with_cpu(snaps, k, lp, where, layer):
    """Instance ``k`` of the walk against dga_cpu at the LP's stops: flags 0, x, y and draws bit for bit.  Returns comparisons made."""
    for s, ref in _references(lp):
        snap = snaps[s]
        order = "the reference's order" if s <= lp.horizon else "the device's order (behind the horizon)"
        at = f"{where}, after {s + 1} iterations (horizon {lp.horizon})"
        _require(int(snap[4][k]) == 0, at + f": status flags {int(snap[4][k])}", layer)
        bad = _instance_equals(snap, k, ref)
        _require(not bad, at + f": {', '.join(bad)} differ from dga_cpu in {order}", layer)
    return len(_references(lp))


def _compare_with_single(snap, report, k, lp, path, where):
    """Instance ``k`` after all iterations against the single solver on it alone, the report's row included."""
    one = single_result(lp, path)
    last = one["snaps"][DGA_ITERS - 1]
    at = f"{where}, after {DGA_ITERS} iterations against DeviceDGA ({path}) alone"
    _require(int(snap[4][k]) == int(last[4][0]), at + f": status flags {int(snap[4][k])} != {int(last[4][0])}")
    if int(last[4][0]) == 0:
        bad = _instance_equals(snap, k, (last[0][0], last[1][0], last[2][0], int(last[3][0])))
        _require(not bad, at + f": {', '.join(bad)} differ")
        _require(tuple(float(v) for v in report[k]) == one["report"], at + f": report {tuple(report[k])} != {one['report']}")


def _check_bound(counts, lp, flags, energy, y_eq, y_ineq, where):
    """The certified lower bound against HiGHS: a clean LP's dual energy does not exceed its optimum by more than its rounding.
    An LP that the device flags has no bound to check; where dga_cpu in the device's order runs clean that is a mismatch, else
    it is counted as skipped."""
    if not lp.clean:
        return
    if int(flags) != 0:
        _require(lp.device_fail is not None, f"{where}: status flags {int(flags)} after {DGA_ITERS} iterations, dga_cpu runs clean in the device's order")
        counts["bounds_skipped"] += 1
        return
    res = lp.linprog()
    _require(res.status == 0, f"{where}: linprog status {res.status} ({res.message})")
    slack = lp.bound_slack(y_eq, y_ineq)
    _require(energy <= res.fun + slack, f"{where}: the dual bound {energy!r} exceeds the optimum {res.fun!r} by more than {slack!r}")
    counts["bounds"] += 1


def _status_step(state, lp, k, check_text, where, neighbours=(), single=False):
    """The raise of dga_cpu in iteration ``t`` on instance ``k``: after ``t`` iterations no flag anywhere and the references'
    iterates, after one more exactly the bit on ``k``, ``check()`` names it, the neighbours unharmed at ``t + 1``."""
    t, name = lp.fail
    bit = STATUS_BITS[name]
    everyone = [(k, lp)] + list(neighbours)
    if t > 0:
        for p in _pieces(t):
            state.iterate(p)
        snap = _snapshot(state, single)
        for i, other in everyone:
            _require(int(snap[4][i]) == 0, f"{where}: flags {int(snap[4][i])} on {i} after {t} iterations, before the raise")
            bad = _instance_equals(snap, i, other.states[t - 1])
            _require(not bad, f"{where}: {', '.join(bad)} of {i} differ from dga_cpu after {t} iterations, before the raise")
    state.iterate(1)
    snap = _snapshot(state, single)
    _require(int(snap[4][k]) == bit, f"{where}: flags {int(snap[4][k])} after iteration {t}, dga_cpu raises '{name}' (bit {bit}) there")
    try:
        state.check()
        raised = None
    except (ValueError, AssertionError) as e:
        raised = str(e)
    _require(raised is not None and name in raised and check_text in raised, f"{where}: check() gave {raised!r}, expected '{name}' {check_text}")
    for i, other in neighbours:
        _require(int(snap[4][i]) == 0, f"{where}: flags {int(snap[4][i])} on the clean neighbour {i} after iteration {t}")
        bad = _instance_equals(snap, i, other.states[t])
        _require(not bad, f"{where}: {', '.join(bad)} of the clean neighbour {i} differ from dga_cpu after {t + 1} iterations")


SINGLE_PATHS = ("fused", "general")
BATCH_PATHS = ("fused", "general-segmented", "general-global")


def run_dga(cases, seed):
    """``DeviceDGA`` on both search paths: instance 0 of every batch of the pool and every LP on which dga_cpu raises, against
    dga_cpu; status bits; the dual bound against HiGHS.  Returns counts."""
    counts = dict(lps=0, comparisons=0, raises=0, bounds=0, bounds_skipped=0)
    for batch in dga_pool(cases, seed):
        chosen = [batch[0]] + [lp for lp in batch[1:] if lp.status_ok][:2]
        for lp in chosen:
            for path in SINGLE_PATHS:
                where = f"dga {lp.name}, path {path}"
                got = single_result(lp, path)
                counts["comparisons"] += _compare_with_cpu(got["snaps"], 0, lp, where, None)
                last = got["snaps"][DGA_ITERS - 1]
                _check_bound(counts, lp, last[4][0], got["report"][0], last[1][0], last[2][0], where)
                if lp.status_ok:
                    with single_state(lp, path) as state:
                        _status_step(state, lp, 0, "", where, single=True)
                    counts["raises"] += 1
            counts["lps"] += 1
    return counts


def run_dga_batch(cases, seed):
    """``DeviceDGABatch`` on its three paths: every instance against dga_cpu and against ``DeviceDGA`` alone (report rows
    included); a raising cost between two clean instances of its batch; the dual bound.  Returns counts."""
    counts = dict(batches=0, instances=0, comparisons=0, raises=0, raises_without_neighbours=0, bounds=0, bounds_skipped=0)
    for case, batch in enumerate(dga_pool(cases, seed)):
        stops = sorted({s for lp in batch for s in lp.stops()} | set(DGA_STOPS))
        for path in BATCH_PATHS:
            one = path.partition("-")[0]
            with batch_state(batch, path) as state:
                snaps = _walk(state, stops)
                report = state.report()
            for k, lp in enumerate(batch):
                where = f"dga_batch {lp.name} of {len(batch)}, path {path}"
                counts["comparisons"] += _compare_with_cpu(snaps, k, lp, where, _dga_single_agrees(lp, one))
                last = snaps[DGA_ITERS - 1]
                _compare_with_single(last, report, k, lp, one, where)
                _check_bound(counts, lp, last[4][k], report[k, 0], last[1][k], last[2][k], where)
        # a raising instance between two instances of its batch that are clean through the iteration of the raise
        for k, lp in enumerate(batch):
            if not lp.status_ok:
                continue
            t = lp.fail[0]
            clean = [other for other in batch if other is not lp and other.clean and other.horizon >= t][:2]
            trio, at, neighbours = [lp], 0, []
            if len(clean) == 2:
                trio, at, neighbours = [clean[0], lp, clean[1]], 1, [(0, clean[0]), (2, clean[1])]
            else:
                counts["raises_without_neighbours"] += 1
            for path in BATCH_PATHS:
                with batch_state(trio, path) as state:
                    _status_step(state, lp, at, f"instances [{at}] of the batch", f"dga_batch status {lp.name}, path {path}", neighbours)
            counts["raises"] += 1
            break   # one per batch
        counts["batches"] += 1
        counts["instances"] += len(batch)
    return counts


def run_dga_many(cases, seed):
    """``DeviceDGAMany`` with the launch length chosen by the library and with one iteration per launch: every LP of every list
    against dga_cpu and against ``DeviceDGA`` alone (report rows included); a raising LP between two clean ones; the dual bound.
    Returns counts."""
    counts = dict(lists=0, lps=0, comparisons=0, raises=0, bounds=0, bounds_skipped=0, longest=0)
    pool = dga_pool(cases, seed)
    for case, lps in enumerate(dga_lists(cases, seed)):
        stops = sorted({s for lp in lps for s in lp.stops()} | set(DGA_STOPS))
        for setting, kmax in (("default", None), ("kmax1", 1)):
            with many_state(lps, kmax) as state:
                _require(kmax is None or state.kmax() == kmax, f"dga_many seed {seed} list {case}: kmax {state.kmax()} under {kmax}")
                snaps = _walk(state, stops)
                report = state.report()
            for k, lp in enumerate(lps):
                where = f"dga_many seed {seed} list {case} LP {k} of {len(lps)} ({lp.name}), setting {setting}"
                counts["comparisons"] += _compare_with_cpu(snaps, k, lp, where, _dga_single_agrees(lp, "fused"))
                last = snaps[DGA_ITERS - 1]
                _compare_with_single(last, report, k, lp, "fused", where)
                _check_bound(counts, lp, last[4][k], report[k, 0], last[1][k], last[2][k], where)
        counts["lists"] += 1
        counts["lps"] += len(lps)
        counts["longest"] = max(counts["longest"], len(lps))
    # every comparable raise of the pool's first instances between two clean LPs of other shapes
    everyone = [lp for batch in pool for lp in batch[:3]]
    for lp in everyone:
        if not lp.status_ok:
            continue
        t = lp.fail[0]
        clean = [other for other in everyone if other.clean and other.horizon >= t and other.args[1] is not lp.args[1]][:2]
        _require(len(clean) == 2, f"dga_many status {lp.name}: the pool has no two clean LPs")
        for setting, kmax in (("default", None), ("kmax1", 1)):
            with many_state([clean[0], lp, clean[1]], kmax) as state:
                _status_step(state, lp, 1, "LPs [1] of the list", f"dga_many status {lp.name}, setting {setting}", [(0, clean[0]), (2, clean[1])])
        counts["raises"] += 1
    return counts


def run_dga_many_stop(cases, seed):
    """``DeviceDGAMany.set_stop`` / ``stop_state`` and ``dual_gradient_ascent_many_until`` on the lists of ``run_dga_many``, armed from
    creation, with the launch length chosen by the library and with one iteration per launch: ``stop_state`` of every compared LP
    with ``==`` against the restatement, its x, y, tie draws and flags against dga_cpu at that LP's own count, its report against
    ``DeviceDGA`` alone where the single solver's walk has that count.  The LPs left out (``DgaStopCase``) are run, not compared;
    their share is asserted.  Returns counts."""
    from pysparselp_amd import dual_gradient_ascent_many_until

    stats = dga_stop_statistics(cases, seed)
    _require(stats["left_out"] <= DGA_STOP_LEFT_OUT * stats["lps"],
             f"dga_many_stop seed {seed}: {stats['left_out']} of {stats['lps']} LPs lie behind their parity horizon, more than a quarter")
    counts = dict(lists=0, runs=0, lps=0, compared=0, left_out=0, stopped=0, running=0, drivers=0, longest=0)
    for no, case in enumerate(dga_stop_cases(cases, seed)):
        lps, known = case.lps, case.compared()
        for setting, kmax in (("default", None), ("kmax1", 1)):
            with many_state(lps, kmax) as state:
                state.set_stop(case.tol, case.every)
                for p in _pieces(DGA_ITERS):
                    state.iterate(p)
                got, snap = state.stop_state(), _snapshot(state)
            for k in known:
                lp, want = lps[k], case.want[k]
                where = (f"dga_many_stop seed {seed} list {no} LP {k} of {len(lps)} ({lp.name}), setting {setting}, tol {case.tol!r} "
                         f"(from {case.source}), every {case.every}")
                mine = (int(got[0][k]), bool(got[1][k]), float(got[2][k]))
                _require(mine == (int(want[0]), bool(want[1]), float(want[2])), where + f": stop_state {mine} != {tuple(want)}",
                         _dga_single_agrees(lp, "fused"))
                _require(int(snap[4][k]) == 0, where + f": status flags {int(snap[4][k])}")
                bad = _instance_equals(snap, k, lp.states[int(want[0]) - 1])
                _require(not bad, where + f": {', '.join(bad)} differ from dga_cpu after {int(want[0])} iterations", _dga_single_agrees(lp, "fused"))
            counts["runs"] += 1
        if all(lp.clean and lp.device_fail is None for lp in lps):   # the driver checks the status of every LP after every call
            xs, y_eqs, _, info = dual_gradient_ascent_many_until([_LP(*lp.args) for lp in lps], case.tol, case.every, nb_max_iter=DGA_ITERS)
            for k in known:
                want = case.want[k]
                where = f"dga_many_stop seed {seed} list {no} LP {k} ({lps[k].name}), dual_gradient_ascent_many_until"
                mine = (int(info["iterations"][k]), bool(info["stopped"][k]), float(info["step"][k]))
                _require(mine == (int(want[0]), bool(want[1]), float(want[2])), where + f": info {mine} != {tuple(want)}")
                ref = lps[k].states[int(want[0]) - 1]
                _require(np.array_equal(xs[k], ref[0]) and np.array_equal(y_eqs[k], ref[1]), where + ": x or y_eq differ from dga_cpu")
            counts["drivers"] += 1
        counts["lists"] += 1
        counts["lps"] += len(lps)
        counts["compared"] += len(known)
        counts["left_out"] += len(lps) - len(known)
        counts["stopped"] += sum(bool(case.want[k][1]) for k in known)
        counts["running"] += sum(not case.want[k][1] for k in known)
        counts["longest"] = max(counts["longest"], len(lps))
    _require(counts["left_out"] <= DGA_STOP_LEFT_OUT * counts["lps"], f"dga_many_stop seed {seed}: {counts['left_out']} of {counts['lps']} LPs left out")
    return counts


DGAB_STOP_NAMES = (("iterations", np.int64), ("stopped", np.bool_), ("step", np.float64), ("bound", np.float64), ("reason", np.int32))


def _dgab_read(state):
    """Everything ``run_dga_batch_stop`` compares of a state: ``(stop_state, snapshot, report, frozen, iterations done)``."""
    return state.stop_state(), _snapshot(state), state.report(), state.frozen(), state.status()[3]


def _dgab_same(p, q):
    return (all(np.array_equal(a, b, equal_nan=True) for a, b in zip(p[0], q[0])) and all(np.array_equal(a, b) for a, b in zip(p[1], q[1]))
            and np.array_equal(p[2], q[2], equal_nan=True) and np.array_equal(p[3], q[3]) and p[4] == q[4])


def _dgab_compare(counts, case, name, total, read, where, path, final):
    """The instances of ``case`` that are known after ``total`` iterations of schedule ``name`` against the restatement and
    dga_cpu: ``stop_state`` with dtypes, x, y, tie draws and flags at the instance's own count, the report's bound against
    ``device_energy`` there, ``frozen()``; a clean LP's record that met its cut-off against HiGHS."""
    got, snap, report, frozen, _ = read
    want, known = case.want(name, total)
    for g, (label, dtype) in zip(got, DGAB_STOP_NAMES):
        _require(g.dtype == dtype and g.shape == (len(case.lps),), f"{where}: {label} has dtype {g.dtype}, shape {g.shape}")
    _require(np.array_equal(frozen, case.frozen), f"{where}: frozen() is {np.flatnonzero(frozen).tolist()}, constructed {case.frozen_at}")
    one = path.partition("-")[0]
    for k in np.flatnonzero(known):
        lp = case.lps[k]
        at = f"{where}, instance {k} of {len(case.lps)} ({lp.name}, horizon {lp.horizon}), after {total} iterations"
        layer = None if case.frozen[k] else _dga_single_agrees(lp, one)
        for g, w, (label, _) in zip(got, want, DGAB_STOP_NAMES):
            _require(np.array_equal(g[k], w[k], equal_nan=True), at + f": {label} {g[k]!r}, restated {w[k]!r} (stop_state "
                     f"{tuple(g[k] for g in got)}, restated {tuple(w[k] for w in want)}, first cut-off "
                     f"{None if case.schedule(name)[0][2] is None else case.schedule(name)[0][2][k]!r})", layer)
        done = int(want[0][k])
        _require(int(snap[4][k]) == 0, at + f": status flags {int(snap[4][k])}", layer)
        bad = _instance_equals(snap, k, lp.states[done - 1])
        _require(not bad, at + f": {', '.join(bad)} differ from dga_cpu after {done} iterations", layer)
        energy = case.bounds(k)[done - 1] if done > 0 else case.start_bound(k)
        _require(np.array_equal(report[k, 0], energy, equal_nan=True),
                 at + f": report()[{k}, 0] = {report[k, 0]!r} after {done} iterations, device_energy {energy!r}", layer)
        counts["reports"] += 1
        if final and want[4][k] & 2:
            _check_bound(counts, lp, snap[4][k], got[3][k], snap[1][k], snap[2][k], at)
    return want, known


def run_dga_batch_stop(cases, seed, paths=BATCH_PATHS):
    """``DeviceDGABatch.set_stop`` / ``stop_state`` and ``dual_gradient_ascent_batch_until`` on batches of their own
    (``dga_batch_stop_cases``), against tests/dga_batch_stop_cpu.py on curves restated on the CPU -- the steps from dga_cpu's
    multipliers, the bounds from ``dga_cpu.device_energy`` on them: schedule A (armed from creation) on each of ``paths``, schedule B
    (armed in mid-life, armed again with other cut-offs and cadence, turned off) on ``fused``.  Every instance inside its parity
    horizon: ``stop_state`` bit for bit with dtypes, x, y, tie draws and flags against dga_cpu at its own count, ``report()[k, 0]``
    against ``device_energy`` there, ``frozen()``, a record that met its cut-off against HiGHS.  The instances left out
    (``DgaBatchStopCase.want``) are run as neighbours; their share is asserted.  Returns counts."""
    stats = dga_batch_stop_statistics(cases, seed)
    _require(stats["left_out"] <= DGA_STOP_LEFT_OUT * stats["instance_schedules"],
             f"dga_batch_stop seed {seed}: {stats['left_out']} of {stats['instance_schedules']} instance-schedules lie behind their parity "
             "horizon, more than a quarter")
    counts = _dgab_counts()
    for case in dga_batch_stop_cases(cases, seed):
        _dgab_run_case(counts, case, seed, paths, "fused")
    _require(counts["left_out"] <= DGA_STOP_LEFT_OUT * counts["instances"],
             f"dga_batch_stop seed {seed}: {counts['left_out']} of {counts['instances']} instance-schedules left out")
    return counts


def run_dga_batch_stop_large(seed, paths=("general-segmented", "general-global")):
    """The same comparisons on ``dga_batch_stop_large_case``, by the general search (schedule B under ``general-global``): the bound
    of the check and of the report where the last workgroup of the column pass holds terms.  Returns counts; no cap."""
    counts = _dgab_counts()
    _dgab_run_case(counts, dga_batch_stop_large_case(seed), seed, paths, "general-global")
    return counts


def _dgab_counts():
    return dict(batches=0, runs=0, instances=0, compared=0, left_out=0, stopped=0, running=0, frozen=0, longest=0, drivers=0, reports=0,
                idle=0, bounds=0, bounds_skipped=0)


def _dgab_run_case(counts, case, seed, paths, both_on):
    """One case of ``run_dga_batch_stop``: schedule A on every path of ``paths``, schedule B on the path ``both_on``, the driver."""
    from pysparselp_amd import dual_gradient_ascent_batch_until

    lps = case.lps
    for path in paths:
        for name in ("A", "B") if path == both_on else ("A",):
            where = f"dga_batch_stop seed {seed} case {case.no}, path {path}, {case.rule_text(name)}"
            rules, phases, done = list(case.schedule(name)), case.phases(name), 0
            with batch_state(lps, path) as state:
                for total in phases:
                    if rules and rules[0][0] == done:
                        _, tol, targets, every = rules.pop(0)
                        state.set_stop(tol, targets, every)
                    for p in _pieces(total - done):
                        state.iterate(p)
                    done = total
                    read = _dgab_read(state)
                    want, known = _dgab_compare(counts, case, name, total, read, where, path, total == DGA_ITERS)
                live = known & ~case.frozen
                if name == "A" and path == both_on and known.all() and (want[1] | case.frozen).all():
                    state.iterate(5)   # nothing moves: no launch, and `iters` stays
                    _require(_dgab_same(read, _dgab_read(state)), f"{where}: iterate(5) on a batch in which nothing moves changed it")
                    counts["idle"] += 1
            counts["runs"] += 1
            counts["instances"] += len(lps)
            counts["compared"] += int(known.sum())
            counts["left_out"] += int((~known).sum())
            counts["stopped"] += int((live & want[1]).sum())
            counts["running"] += int((live & ~want[1]).sum())
            counts["frozen"] += int((known & case.frozen).sum())
        # the driver checks the status of every instance after every call, and a frozen instance needs no driver
        if case.frozen_at is None and all(lp.clean and lp.device_fail is None for lp in lps):
            one, _, sort = path.partition("-")
            (want, known), (_, tol, targets, every) = case.want("A"), case.rules_a[0]
            with environment(SLP_DGA_BATCH_SORT=sort or None):
                xs, y_eqs, y_ineqs, info = dual_gradient_ascent_batch_until(
                    _LP(*lps[0].args), np.array([lp.args[0] for lp in lps]), tol, targets, every, nb_max_iter=DGA_ITERS,
                    lower_bounds=np.array([lp.args[5] for lp in lps]), upper_bounds=np.array([lp.args[6] for lp in lps]), path=one)
            for k in np.flatnonzero(known):
                at = f"dga_batch_stop seed {seed} case {case.no} instance {k} ({lps[k].name}), path {path}, dual_gradient_ascent_batch_until, {case.rule_text('A')}"
                mine = (info["iterations"][k], info["stopped"][k], info["step"][k], info["reason"][k])
                theirs = (want[0][k], want[1][k], want[2][k], want[4][k])
                _require(all(np.array_equal(g, w, equal_nan=True) for g, w in zip(mine, theirs)), at + f": info {mine} != {theirs}")
                ref = lps[k].states[int(want[0][k]) - 1]
                _require(np.array_equal(xs[k], ref[0]) and np.array_equal(y_eqs[k], ref[1])
                         and (ref[2] is None or np.array_equal(y_ineqs[k], ref[2])), at + ": x or y differ from dga_cpu")
                energy = case.bounds(k)[int(want[0][k]) - 1]
                _require(np.array_equal(info["lower_bound"][k], energy, equal_nan=True),
                         at + f": lower_bound {info['lower_bound'][k]!r}, device_energy {energy!r}")
            counts["drivers"] += 1
    counts["batches"] += 1
    counts["longest"] = max(counts["longest"], len(lps))


FAMILIES = {"cp_batch": run_cp_batch, "cp_many": run_cp_many, "admm_batch": run_admm_batch, "admm_many": run_admm_many, "dga": run_dga,
            "dga_batch": run_dga_batch, "dga_many": run_dga_many, "cp_many_stop": run_cp_many_stop, "admm_many_stop": run_admm_many_stop,
            "dga_many_stop": run_dga_many_stop, "cp_many_gap": run_cp_many_gap, "cp_batch_gap": run_cp_batch_gap,
            "admm_batch_stop": run_admm_batch_stop,
            "dga_batch_stop": lambda cases, seed: dict(run_dga_batch_stop(cases, seed), large_case=run_dga_batch_stop_large(seed))}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cases", type=int, default=TEST_CASES)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--family", default=",".join(FAMILIES), help="comma-separated, among " + ", ".join(FAMILIES) + " (default: all)")
    args = p.parse_args()
    failed = 0
    for name in args.family.split(","):
        try:
            print("ok:", name, FAMILIES[name](args.cases, args.seed), flush=True)
        except AssertionError as e:
            failed += 1
            print("MISMATCH:", name, e, flush=True)
    sys.exit(3 if failed else 0)   # (1 is Python's own: an exception that is no mismatch)


if __name__ == "__main__":
    main()
