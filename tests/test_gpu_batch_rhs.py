"""Right-hand sides per instance for the batched dual gradient ascent and the batched ADMM solver on the GPU
(``DeviceDGABatch.set_rhs`` / ``dual_gradient_ascent_batch_rhs`` / ``SparseLP.solve_dga_batch_rhs``; ``ADMMBatchState.set_rhs`` /
``lp_admm_batch_rhs`` / ``SparseLP.solve_admm_batch_rhs``).

The contract: instance k is BIT FOR BIT what the single solver computes on a copy of the LP whose right-hand sides are row k --
``DeviceDGA`` (x, y, the tie draws taken, the flags, the report's three numbers) and ``ADMMState.from_lp(...,
order=ORDER_SEQUENTIAL)`` / ``oracle.lp_admm`` (x over all N columns, lambda, the violations; the energy, a sum in another order,
to ``ENERGY_TOL`` of tests/test_gpu_admm_batch.py), at a fixed horizon and, with a stopping test, at the instance's own stopping
iteration.

Instance 0 has the fixture's own right-hand sides; instance k >= 1 perturbs every finite entry by ``0.1 (1 + |b|) randn`` --
``b_upper`` only upwards, ``b_lower`` only downwards, infinite entries stay -- and one row of one instance has
``b_lower == b_upper``.  Feasibility is not needed: iterates are compared with iterates.  The instances also differ in their costs,
so that they differ from each other shows nothing about the right-hand sides; the comparisons against the single solver therefore
also check, per varied side, that instance k >= 1 with the FIXTURE's own sides gives other iterates than the batch's instance k:
a kernel that reads instance 0's vector everywhere cannot pass.  Needs a real MI355X: run with ``-m gpu``."""
import copy
import functools

import numpy as np
import pytest

from conftest import Recorder, load_golden, lp_from_golden, solver_args
from dga_batch_cases import REMAINDER_SIZES, STOPS, batch_case
from dga_cpu import dga_cpu, dual_argmin, dual_energy
from oracle import oracle
from test_gpu_admm_batch import ENERGY_TOL, BatchRecorder, _instances, form  # noqa: F401  (``form``: the fixture of both forms)
from test_gpu_dga import LP, device_state
from test_gpu_dga_batch import PATHS, batch_state, snapshot

pytestmark = pytest.mark.gpu

ITERS = 30


def perturbed(b, batch, rs, direction=0):
    """``(batch, rows)``: row 0 is ``b``; row k >= 1 moves every finite entry by ``0.1 (1 + |b|) randn`` -- upwards only with
    ``direction > 0``, downwards only with ``direction < 0``."""
    b = np.asarray(b, dtype=np.float64)
    out = np.tile(b, (batch, 1))
    move = 0.1 * (1 + np.abs(np.where(np.isfinite(b), b, 0.0))) * rs.randn(batch - 1, b.size)
    if direction:
        move = direction * np.abs(move)
    out[1:] = np.where(np.isfinite(b), b + move, b)
    return out


def all_differ(rows):
    return all(not np.array_equal(rows[i], rows[j]) for i in range(len(rows)) for j in range(i))


# =============================================================================================================== dual ascent
DGA_CASES = ("potts8", "sc50a", "random1")
DGA_B = 5


@functools.lru_cache(maxsize=None)
def dga_rhs(case, batch=DGA_B):
    """``(args, costs, b_eq[batch, m_eq], b_upper[batch, m_ineq])`` (never modified)."""
    args, six = batch_case(case)
    rs = np.random.RandomState(31 + len(case))
    costs = np.tile(six, (batch // 6 + 1, 1))[:batch]
    return args, costs, perturbed(args[2], batch, rs), perturbed(args[4], batch, rs, +1)


def dga_instance_args(args, costs, be, bu, k):
    """The single solver's arguments for instance k; ``be`` / ``bu`` 1-D (shared) or 2-D."""
    pick = lambda v: v if np.ndim(v) == 1 else v[k]  # noqa: E731
    return (costs[k], args[1], pick(be), args[3], pick(bu), args[5], args[6])


def stacked(be, bu, batch):
    """The rows of ``[b_eq; b_upper]`` as ``set_rhs`` takes them."""
    if np.ndim(be) == 1 and np.ndim(bu) == 1:
        return np.concatenate((be, bu))
    return np.ascontiguousarray(np.concatenate((np.broadcast_to(be, (batch, np.shape(be)[-1])), np.broadcast_to(bu, (batch, np.shape(bu)[-1]))), axis=1))


def single_result(iargs, path, iters):
    """``(x, y_eq, y_ineq, draws, flags, report)`` of ``DeviceDGA`` after ``iters`` iterations."""
    single, smat = device_state(iargs, path.partition("-")[0])
    try:
        single.iterate(iters)
        flags, draws, _, _ = single.status()
        return (single.x(), *single.y(), draws, flags, single.report())
    finally:
        single.close()
        smat.close()


def assert_same_instance(snap, report, k, ref, what):
    x, y_eq, y_ineq, draws, flags, _ = snap
    assert np.array_equal(x[k], ref[0]) and np.array_equal(y_eq[k], ref[1]) and np.array_equal(y_ineq[k], ref[2]), what
    assert draws[k] == ref[3] and flags[k] == ref[4], what
    if report is not None:
        assert tuple(report[k]) == tuple(ref[5]), what


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", DGA_CASES)
def test_dga_every_instance_equals_the_single_solver_on_its_own_right_hand_sides(case, path):
    """B = 5: both kinds of rows batched, then the equality rows alone, then the inequality rows alone."""
    args, costs, bes, bus = dga_rhs(case)
    for which, be, bu in (("both", bes, bus), ("eq", bes, args[4]), ("upper", args[2], bus)):
        state, mat = batch_state(args, costs, path)
        try:
            state.set_rhs(stacked(be, bu, DGA_B))
            state.iterate(ITERS)
            snap, report = snapshot(state), state.report()
        finally:
            state.close()
            mat.close()
        assert snap[5] == ITERS
        for k in range(DGA_B):
            ref = single_result(dga_instance_args(args, costs, be, bu, k), path, ITERS)
            assert_same_instance(snap, report, k, ref, (case, path, which, k))
        # the same costs with the fixture's own right-hand sides give other multipliers: the instance's rows were read
        if np.size({"both": stacked(args[2], args[4], 1), "eq": args[2], "upper": args[4]}[which]):   # the varied kind has rows
            for k in range(1, DGA_B):
                own = single_result(dga_instance_args(args, costs, args[2], args[4], k), path, ITERS)
                assert not (np.array_equal(own[1], snap[1][k]) and np.array_equal(own[2], snap[2][k])), (case, path, which, k)


@pytest.mark.parametrize("path", PATHS)
def test_dga_instances_equal_the_cpu_restatement(path):
    """SC50A against tests/dga_cpu.py in the reference's order of sums, each instance with its own right-hand sides, at every entry
    of ``STOPS``: after 1, 2, 11, 51 and 101 iterations, the horizon of tests/test_gpu_dga_batch.py."""
    args, costs, bes, bus = dga_rhs("sc50a")
    keep = STOPS
    assert max(keep) == 100
    state, mat = batch_state(args, costs, path)
    try:
        state.set_rhs(stacked(bes, bus, DGA_B))
        snaps, done = {}, 0
        for it in keep:
            state.iterate(it + 1 - done)
            done = it + 1
            snaps[it] = snapshot(state)
    finally:
        state.close()
        mat.close()
    for k in range(DGA_B):
        ref = dga_cpu(costs[k], args[1], bes[k], args[3], bus[k], args[5], args[6], nb_max_iter=max(keep) + 1, order="reference", keep=keep)
        for it in keep:
            x, y_eq, y_ineq, draws, flags, _ = snaps[it]
            assert flags[k] == 0
            assert np.array_equal(x[k], ref[it][0]) and np.array_equal(y_eq[k], ref[it][1]) and np.array_equal(y_ineq[k], ref[it][2]), (k, it)
            assert draws[k] == ref[it][3], (k, it)


DISTINCT = 7


@functools.lru_cache(maxsize=None)
def dga_remainder_reference(path):
    """Seven distinct (cost, right-hand side) pairs on Potts-8, each solved in a batch of ONE with ``set_rhs``."""
    args, costs, bes, bus = dga_rhs("potts8", DISTINCT)
    out = []
    for k in range(DISTINCT):
        state, mat = batch_state(args, costs[k:k + 1], path)
        try:
            state.set_rhs(stacked(bes[k:k + 1], bus[k:k + 1], 1))
            state.iterate(ITERS)
            snap, report = snapshot(state), state.report()
            out.append((snap[0][0], snap[1][0], snap[2][0], snap[3][0], snap[4][0], report[0]))
        finally:
            state.close()
            mat.close()
    return out


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("batch", REMAINDER_SIZES)
def test_dga_batch_sizes_around_the_tile_of_64_repeat_seven_right_hand_sides(batch, path):
    args, costs, bes, bus = dga_rhs("potts8", DISTINCT)
    ref = dga_remainder_reference(path)
    order = np.arange(batch) % DISTINCT
    state, mat = batch_state(args, costs[order], path)
    try:
        state.set_rhs(stacked(bes[order], bus[order], batch))
        state.iterate(ITERS)
        snap, report = snapshot(state), state.report()
    finally:
        state.close()
        mat.close()
    for k in range(batch):
        assert_same_instance(snap, report, k, ref[order[k]], (batch, path, k))
    assert all_differ([np.concatenate((r[1], r[2])) for r in ref])
    if batch == 1:   # and the batch of one is the single solver
        assert_same_instance(snap, report, 0, single_result(dga_instance_args(args, costs, bes, bus, 0), path, ITERS), path)


def driver_path(monkeypatch, path):
    """The ``path`` argument of the drivers for an entry of ``PATHS``; the sort of the general search goes through the environment."""
    path, _, sort = path.partition("-")
    if sort:
        monkeypatch.setenv("SLP_DGA_BATCH_SORT", sort)
    return path


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", DGA_CASES)
def test_dga_with_cut_offs_every_instance_is_its_single_solve_to_its_own_stopping_iteration(case, path, monkeypatch):
    """B = 6.  The cut-offs of instances 1 and 4 are their own bounds after 10 iterations, taken from a dry run, so that they
    retire at the first check while their neighbours run on: an instance's place in the batch, not its place among the instances
    still moving, must pick its right-hand sides."""
    from pysparselp_amd import dual_gradient_ascent_batch_rhs
    from pysparselp_amd.DualGradientAscent import dual_gradient_ascent

    args, costs, bes, bus = dga_rhs(case, 6)
    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = args
    state, mat = batch_state(args, costs, path)
    try:
        state.set_rhs(stacked(bes, bus, 6))
        state.iterate(10)
        bound10 = state.report()[:, 0]
        state.iterate(ITERS - 10)
        bound30 = state.report()[:, 0]
    finally:
        state.close()
        mat.close()
    assert np.all(np.isfinite(bound10))
    drv = driver_path(monkeypatch, path)
    targets = np.full(6, np.inf)
    targets[[1, 4]] = bound10[[1, 4]]
    lp = LP(c, a_eq, b_eq, a_ineq, b_upper, lb, ub)
    x, y_eq, y_ineq, info = dual_gradient_ascent_batch_rhs(lp, costs, bes, bus, targets=targets, check_every=10, nb_max_iter=ITERS, path=drv)
    print(case, path, "bounds at 10", bound10, "iterations", info["iterations"])
    assert info["iterations"].tolist() == [ITERS, 10, ITERS, ITERS, 10, ITERS]
    assert info["stopped"].tolist() == [False, True, False, False, True, False] and info["reason"].tolist() == [0, 2, 0, 0, 2, 0]
    assert np.array_equal(info["lower_bound"], np.where(info["stopped"], bound10, bound30))
    for k in range(6):
        one = dual_gradient_ascent(None, LP(costs[k], a_eq, bes[k], a_ineq, bus[k], lb, ub), nb_max_iter=int(info["iterations"][k]))
        assert np.array_equal(x[k], one[0]) and np.array_equal(y_eq[k], one[1]) and np.array_equal(y_ineq[k], one[2]), (case, path, k)
    # the step test reads no right-hand side, but its instances go through the same launches
    x2, ye2, yi2, info2 = dual_gradient_ascent_batch_rhs(lp, costs, bes, bus, tol=0.0, check_every=10, nb_max_iter=ITERS, path=drv)
    assert info2["iterations"].tolist() == [ITERS] * 6 and not info2["stopped"].any()
    fixed = dual_gradient_ascent_batch_rhs(lp, costs, bes, bus, nb_max_iter=ITERS, path=drv)
    assert np.array_equal(x2, fixed[0]) and np.array_equal(ye2, fixed[1]) and np.array_equal(yi2, fixed[2])
    assert np.array_equal(fixed[3]["lower_bound"], bound30) and fixed[3]["iterations"].tolist() == [ITERS] * 6
    assert not fixed[3]["stopped"].any() and not fixed[3]["reason"].any()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", DGA_CASES)
def test_dga_a_shared_right_hand_side_and_identical_rows_are_the_shared_run(case, path, monkeypatch):
    from pysparselp_amd import dual_gradient_ascent_batch, dual_gradient_ascent_batch_rhs

    args, costs, _, _ = dga_rhs(case)
    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = args
    state, mat = batch_state(args, costs, path)   # (checks that the path and the sort are the ones asked for)
    state.close()
    mat.close()
    drv = driver_path(monkeypatch, path)
    lp = LP(c, a_eq, b_eq, a_ineq, b_upper, lb, ub)
    want = dual_gradient_ascent_batch(lp, costs, nb_max_iter=ITERS, path=drv)
    other = LP(c, a_eq, 2.0 * b_eq, a_ineq, b_upper + 1.0, lb, ub)   # the LP's own sides are defaults only
    for be, bu in ((b_eq, b_upper), (np.tile(b_eq, (DGA_B, 1)), b_upper), (b_eq, np.tile(b_upper, (DGA_B, 1))),
                   (np.tile(b_eq, (DGA_B, 1)), np.tile(b_upper, (DGA_B, 1)))):
        got = dual_gradient_ascent_batch_rhs(other, costs, be, bu, nb_max_iter=ITERS, path=drv)
        assert all(np.array_equal(g, w) for g, w in zip(got[:3], want)), (np.ndim(be), np.ndim(bu))
    got = dual_gradient_ascent_batch_rhs(lp, costs, nb_max_iter=ITERS, path=drv)   # both default to the LP's
    assert all(np.array_equal(g, w) for g, w in zip(got[:3], want))
    # a 1-D vector through the state's own call, twice, after a batched one
    state, mat = batch_state(args, costs, path)
    try:
        state.set_rhs(np.tile(np.concatenate((2.0 * b_eq, b_upper + 1.0)), (DGA_B, 1)))
        state.set_rhs(np.concatenate((b_eq, b_upper)))
        state.set_rhs(np.concatenate((b_eq, b_upper)))
        state.iterate(ITERS)
        assert np.array_equal(state.x(), want[0]) and np.array_equal(state.y()[0], want[1]) and np.array_equal(state.y()[1], want[2])
    finally:
        state.close()
        mat.close()


def test_dga_set_rhs_after_the_first_iteration_is_refused_and_changes_nothing():
    from pysparselp_amd import SlpError

    args, costs, bes, bus = dga_rhs("sc50a")
    results = []
    for attempt in (False, True):
        state, mat = batch_state(args, costs, "fused")
        try:
            state.set_rhs(stacked(bes, bus, DGA_B))
            state.iterate(1)
            if attempt:
                with pytest.raises(SlpError, match="before the first iteration"):
                    state.set_rhs(stacked(bes[::-1].copy(), bus[::-1].copy(), DGA_B))
                with pytest.raises(SlpError, match="before the first iteration"):
                    state.set_rhs(np.concatenate((args[2], args[4])))
            state.iterate(ITERS - 1)
            results.append((snapshot(state), state.report()))
        finally:
            state.close()
            mat.close()
    for a, b in zip(results[0][0], results[1][0]):
        assert np.array_equal(a, b)
    assert np.array_equal(results[0][1], results[1][1])


def test_solve_dga_batch_rhs_equals_solve_per_instance():
    """Potts-8, B = 3, 201 iterations: x and every curve bit for bit ``solve`` on a copy of the LP with instance k's right-hand
    sides; the certified bound against numpy's dual energy of the returned multipliers within the bound derived in
    tests/test_gpu_dga_batch.py::test_gpu_solve_dga_batch_curves_solutions_and_certified_bounds (2 (n + m + 2) u (S_x + S_y))."""
    from pysparselp_amd.SparseLP import SparseLP

    d = load_golden("lp_potts8")
    lp = lp_from_golden(d, SparseLP)
    args, costs, bes, bus = dga_rhs("potts8", 3)
    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = args
    x, elapsed = lp.solve_dga_batch_rhs(costs, b_equalities=bes, b_upper=bus, nb_iter=201, ground_truth=d["gt"],
                                        ground_truth_indices=d["gt_idx"])
    assert x.shape == (3, c.size) and elapsed > 0 and lp.itrn_curve == [0, 100, 200]
    y_eq, y_ineq = lp.dual_multipliers
    info = lp.stop_info
    assert info["iterations"].tolist() == [201] * 3 and not info["stopped"].any()
    assert np.array_equal(info["lower_bound"], lp.dual_lower_bounds)
    n, m = c.size, a_eq.shape[0] + a_ineq.shape[0]
    for k in range(3):
        one = copy.deepcopy(lp)
        one.costsvector, one.b_equalities, one.b_upper = costs[k].copy(), bes[k].copy(), bus[k].copy()
        xk = one.solve(method="dual_gradient_ascent", get_timing=False, nb_iter=201, ground_truth=d["gt"], ground_truth_indices=d["gt_idx"])
        assert np.array_equal(x[k], xk), k
        assert one.itrn_curve == lp.itrn_curve
        for name in ("pobj_curve", "dobj_curve", "max_violated_constraint", "distance_to_ground_truth", "distanceToGroundTruthAfterRounding"):
            assert [v[k] for v in getattr(lp, name)] == list(getattr(one, name)), (name, k)
        want = dual_energy(costs[k], a_eq, bes[k], a_ineq, bus[k], lb, ub, y_eq[k], y_ineq[k])
        c_bar, _ = dual_argmin(costs[k], a_eq, a_ineq, lb, ub, y_eq[k], y_ineq[k])
        s_x = np.sum(np.abs(np.minimum(c_bar * ub, c_bar * lb)[c_bar != 0]))
        s_y = np.sum(np.abs(y_eq[k] * bes[k])) + np.sum(np.abs(y_ineq[k] * bus[k]))
        bound = 2 * (n + m + 2) * 2.0 ** -53 * (s_x + s_y)
        print(k, "dual bound", lp.dual_lower_bounds[k], "numpy", want, "difference", abs(lp.dual_lower_bounds[k] - want), "allowed", bound)
        assert np.isfinite(want) and abs(lp.dual_lower_bounds[k] - want) <= bound, k
    assert all_differ(np.concatenate((y_eq, y_ineq), axis=1)) and len(set(np.array(lp.max_violated_constraint)[-1].tolist())) == 3
    # with a cut-off the tuple and the attributes are those of solve_dga_batch_until
    targets = np.array([np.inf, lp.dual_lower_bounds[1] - 1e6, np.inf])
    x2 = lp.solve_dga_batch_rhs(costs, b_equalities=bes, b_upper=bus, targets=targets, check_every=5, nb_iter=20, get_timing=False)
    assert x2.shape == x.shape and lp.stop_info["iterations"].tolist() == [20, 5, 20] and lp.stop_info["reason"].tolist() == [0, 2, 0]


# =============================================================================================================== ADMM
ADMM_B = 4


def _mods():
    from pysparselp_amd import ORDER_SEQUENTIAL, ADMMBatchState, lp_admm_batch, lp_admm_batch_rhs
    from pysparselp_amd.ADMM import ADMMState

    return ADMMBatchState, lp_admm_batch, lp_admm_batch_rhs, ADMMState, ORDER_SEQUENTIAL


def admm_case(case):
    d = load_golden("lp_" + case.partition("-")[0])
    return d


@functools.lru_cache(maxsize=None)
def admm_instances(case, vary, batch=ADMM_B):
    """The arguments of ``lp_admm_batch_rhs`` as a dict (never modified).  ``vary``: which of ``beq``, ``b_lower``, ``b_upper`` differ
    per instance (the others stay the fixture's 1-D ones), and ``"all"``: the three of them with batched costs, bounds and start.
    ``case`` ending in ``-noeq`` drops the equality block.  A fixture without a finite ``b_lower`` gets, where that side varies, rows that
    mix -inf and finite entries (instance 0 stays all -inf: the fixture's own)."""
    d = admm_case(case)
    everything = vary == "all"
    args = dict(_instances(d, batch, seed=len(case) + 5, vary=("c", "bounds", "x0") if everything else ("c",)))
    if case.endswith("-noeq"):
        args["a_eq"], args["beq"] = None, None
    rs = np.random.RandomState(7 + len(case) + len(vary))
    bu = np.asarray(args["b_upper"], dtype=np.float64)
    if args["beq"] is not None and (everything or vary == "beq"):
        args["beq"] = perturbed(args["beq"], batch, rs)
    if everything or vary == "b_upper":
        args["b_upper"] = perturbed(bu, batch, rs, +1)
    if everything or vary == "b_lower":
        if args["b_lower"] is None or not np.any(np.isfinite(args["b_lower"])):
            bl = np.full((batch, bu.size), -np.inf)
            rows = np.flatnonzero(np.isfinite(bu))
            for k in range(1, batch):
                some = rows[rs.rand(rows.size) < 0.5]
                bl[k, some] = bu[some] - (1 + np.abs(bu[some])) * (0.5 + rs.rand(some.size))
            args["b_lower"] = bl
        else:
            args["b_lower"] = perturbed(args["b_lower"], batch, rs, -1)
    if everything:   # one row of one instance is an equation
        row = int(np.flatnonzero(np.isfinite(bu))[0])
        args["b_lower"] = args["b_lower"].copy()
        args["b_lower"][2, row] = args["b_upper"][2, row]
    lo = -np.inf if args["b_lower"] is None else args["b_lower"]
    assert np.all(np.broadcast_to(lo, (batch, bu.size)) <= np.broadcast_to(args["b_upper"], (batch, bu.size)))
    return args


def pick(v, k):
    return v if (v is None or np.ndim(v) == 1) else v[k]


def admm_instance(args, k):
    """The single solver's positional arguments and start for instance k."""
    return ((args["cs"][k], args["a_eq"], pick(args["beq"], k), args["a_ineq"], pick(args["b_lower"], k), pick(args["b_upper"], k),
             pick(args["lb"], k), pick(args["ub"], k)), pick(args["x0"], k))


def admm_state(args, how="set_rhs"):
    """An ``ADMMBatchState`` created with instance 0's sides, the batched ones handed to ``set_rhs``."""
    first = {name: pick(args[name], 0) for name in ("beq", "b_lower", "b_upper")}
    st = _mods()[0](args["cs"], args["a_eq"], first["beq"], args["a_ineq"], first["b_lower"], first["b_upper"], args["lb"], args["ub"],
                    args["x0"])
    batched = {name: args[name] for name in first if args[name] is not None and np.ndim(args[name]) == 2}
    try:
        if batched:
            st.set_rhs(**batched)
    except BaseException:
        st.close()
        raise
    return st


def admm_state_result(args, iters):
    """(x over all N, lambda, report) after ``iters`` iterations and the sweep of the next one, as ``_state_result`` of the batch
    tests."""
    st = admm_state(args)
    try:
        st.iterate(iters)
        st.sweep_step()
        return st.x(), st.lam(), st.report()
    finally:
        st.close()


def admm_run(args, **kw):
    return _mods()[2](args["cs"], args["a_eq"], args["beq"], args["a_ineq"], args["b_lower"], args["b_upper"], args["lb"], args["ub"],
                      x0=args["x0"], **kw)


def single_admm(args, k, iters):
    """(x over N, lambda, report) of ``ADMMState.from_lp`` in SEQUENTIAL order after ``iters`` iterations and the next sweep."""
    _, _, _, ADMMState, seq = _mods()
    (c, a_eq, beq, a_ineq, bl, bu, lb, ub), x0 = admm_instance(args, k)
    st = ADMMState.from_lp(c, a_eq, beq, a_ineq, bl, bu, lb, ub, x0, 2, 3, True, order=seq)
    try:
        st.iterate(iters)
        st.sweep_step()
        return st.x(), st.lam(), st.report()[:3]
    finally:
        st.close()


@functools.lru_cache(maxsize=None)
def admm_oracle(case, vary):
    """Per instance the oracle's callbacks of every iteration and its final x (shared by both forms)."""
    args = admm_instances(case, vary)
    out = []
    for k in range(ADMM_B):
        pos, x0 = admm_instance(args, k)
        rec = Recorder()
        out.append((rec, oracle.lp_admm(*pos, x0=x0, nb_iter=ITERS, callback_func=rec, nb_iter_plot=1)))
    return out


@functools.lru_cache(maxsize=None)
def admm_oracle_own_sides(case, vary):
    """Per instance the oracle's final x for the instance's costs, bounds and start with the FIXTURE's own right-hand sides (those
    of instance 0)."""
    args = admm_instances(case, vary)
    own = dict(args, **{name: pick(args[name], 0) for name in ("beq", "b_lower", "b_upper")})
    out = []
    for k in range(ADMM_B):
        pos, x0 = admm_instance(own, k)
        out.append(oracle.lp_admm(*pos, x0=x0, nb_iter=ITERS, nb_iter_plot=ITERS + 1))
    return out


ADMM_CASES = ["potts8", "sc105", "random1", "random1-noeq"]


@pytest.mark.parametrize("vary", ["beq", "b_lower", "b_upper", "all"])
@pytest.mark.parametrize("case", ADMM_CASES)
def test_admm_every_instance_equals_the_oracle_and_the_single_solver(case, vary, form):  # noqa: F811
    key = "b_upper" if (vary == "beq" and case.endswith("-noeq")) else vary   # no equality block: the upper side alone instead
    args = admm_instances(case, key)
    rec = BatchRecorder()
    x, info = admm_run(args, nb_iter=ITERS, callback_func=rec, nb_iter_plot=1)
    assert info is None
    xs, lams, rep = admm_state_result(args, ITERS)
    for k, (ref, xo) in enumerate(admm_oracle(case, key)):
        assert rec.it == ref.it
        assert np.array_equal(np.array(rec.x)[:, k], np.array(ref.x)), k
        assert np.array_equal(x[k], xo), k
        assert np.array_equal(np.array(rec.veq)[:, k], np.asarray(ref.veq, dtype=np.float64)), k
        assert np.array_equal(np.array(rec.vineq)[:, k], np.asarray(ref.vineq, dtype=np.float64)), k
        np.testing.assert_allclose(np.array(rec.e1)[:, k], ref.e1, **ENERGY_TOL)
        sx, sl, sr = single_admm(args, k, ITERS)
        assert np.array_equal(xs[k], sx) and np.array_equal(lams[k], sl), k
        assert np.array_equal(rep[k, 1:], sr[1:]), k
        np.testing.assert_allclose(rep[k, 0], sr[0], **ENERGY_TOL)
    # the instance's own sides were read: with the fixture's sides the same costs, bounds and start give another x
    own = admm_oracle_own_sides(case, key)
    moved = [k for k in range(1, ADMM_B) if not np.array_equal(own[k], x[k])]
    assert moved or (key == "beq" and args["beq"] is None), (case, key)   # (Potts-8 has no equality rows: nothing to vary there)
    if key == "all":
        assert args["lb"].ndim == 2 and args["x0"].ndim == 2 and np.any(args["b_lower"][2] == args["b_upper"][2])


def test_admm_no_lower_side_with_a_batched_upper_side_and_a_lower_side_mixing_infinite_and_finite_rows(form):  # noqa: F811
    d = load_golden("lp_random1")
    assert not np.any(np.isfinite(solver_args(d)[4]))   # the fixture has no finite b_lower
    args = dict(admm_instances("random1", "b_upper"), b_lower=None)
    assert args["b_upper"].ndim == 2
    xs, lams, _ = admm_state_result(args, ITERS)
    for k in range(ADMM_B):
        sx, sl, _ = single_admm(args, k, ITERS)
        assert np.array_equal(xs[k], sx) and np.array_equal(lams[k], sl), k
    args = admm_instances("random1", "b_lower")
    bl = args["b_lower"]
    assert np.all(np.isinf(bl[0])) and all(np.any(np.isinf(bl[k])) and np.any(np.isfinite(bl[k])) for k in range(1, ADMM_B))
    xs, lams, _ = admm_state_result(args, ITERS)
    for k in range(ADMM_B):
        sx, sl, _ = single_admm(args, k, ITERS)
        assert np.array_equal(xs[k], sx) and np.array_equal(lams[k], sl), k
    assert all_differ(xs)


TILE_DISTINCT = 17


def take(args, order):
    return {name: (v[order] if (v is not None and np.ndim(v) == 2 and name not in ("a_eq", "a_ineq")) else v) for name, v in args.items()}


@functools.lru_cache(maxsize=None)
def admm_tile_reference(form_name, tile):
    """17 distinct instances (all three sides, costs, bounds and start differ), each solved in a batch of ONE."""
    args = admm_instances("potts8", "all", TILE_DISTINCT)
    return args, [admm_state_result(take(args, np.array([k])), ITERS) for k in range(TILE_DISTINCT)]


@pytest.mark.parametrize("batch", [1, 5, 17])
@pytest.mark.parametrize("tile", [1, 4, 16])
def test_admm_tile_edges(tile, batch, form, monkeypatch):  # noqa: F811
    """The last tile is partial at every width; each instance equals its run in a batch of one."""
    monkeypatch.setenv("SLP_ADMM_BATCH_TILE", str(tile))
    args, ref = admm_tile_reference(form, tile)
    order = np.arange(batch) % TILE_DISTINCT
    x, lam, rep = admm_state_result(take(args, order), ITERS)
    assert x.shape[0] == batch
    for k in range(batch):
        xs, ls, rs = ref[order[k]]
        assert np.array_equal(x[k], xs[0]) and np.array_equal(lam[k], ls[0]), k
        assert np.array_equal(rep[k, 1:], rs[0, 1:]), k
        np.testing.assert_allclose(rep[k, 0], rs[0, 0], **ENERGY_TOL)
    assert all_differ([r[0][0] for r in ref])
    if batch == 1:   # and the batch of one is the single solver
        sx, sl, _ = single_admm(args, 0, ITERS)
        assert np.array_equal(x[0], sx) and np.array_equal(lam[0], sl)


@pytest.mark.parametrize("case", ADMM_CASES)
def test_admm_with_a_stopping_test_a_stopped_instance_is_the_single_state_at_its_stopping_iteration(case, form):  # noqa: F811
    """B = 6, tolerances from a dry run so that some but not all instances stop inside 60 iterations."""
    ADMMBatchState, _, lp_admm_batch_rhs, ADMMState, seq = _mods()
    args = admm_instances(case, "all", 6)
    horizon, every = 60, 5
    st = admm_state(args)
    try:   # the dry run: a test nothing meets records residual and step at every check
        st.set_stop(0.0, 0.0, every)
        curve = []
        for _ in range(horizon // every):
            st.iterate(every)
            _, _, residual, step = st.stop_state()
            curve.append((residual.copy(), step.copy()))
    finally:
        st.close()
    # every step passes; the residual tolerance lies halfway between two neighbours among the instances' best residuals, three of
    # the six below it where those two differ
    tol_step = 2.0 * float(np.max([s for _, s in curve]))
    best = np.sort(np.min([r for r, _ in curve], axis=0))
    split = [j for j in (3, 2, 4, 1, 5) if best[j - 1] < best[j]]
    assert split, best
    tol_residual = float(0.5 * (best[split[0] - 1] + best[split[0]]))
    assert best[split[0] - 1] <= tol_residual < best[split[0]]
    st = admm_state(args)
    try:
        st.set_stop(tol_residual, tol_step, every)
        st.iterate(horizon)
        iterations, stopped, _, _ = st.stop_state()
        x, lam = st.x(), st.lam()
    finally:
        st.close()
    print(case, form, "tolerances", tol_residual, tol_step, "iterations", iterations, "stopped", stopped)
    assert stopped.any() and not stopped.all()
    for k in range(6):
        (c, a_eq, beq, a_ineq, bl, bu, lb, ub), x0 = admm_instance(args, k)
        one = ADMMState.from_lp(c, a_eq, beq, a_ineq, bl, bu, lb, ub, x0, 2, 3, True, order=seq)
        try:
            one.iterate(int(iterations[k]))
            assert np.array_equal(x[k], one.x()) and np.array_equal(lam[k], one.lam()), (case, k, iterations[k])
        finally:
            one.close()
    # through the driver: the same stopping iterations
    _, info = admm_run(args, tol_residual=tol_residual, tol_step=tol_step, check_every=every, nb_iter=horizon - 1)
    assert np.array_equal(info["iterations"], iterations) and np.array_equal(info["stopped"], stopped)


def test_admm_a_shared_right_hand_side_and_identical_rows_are_the_shared_run(form):  # noqa: F811
    _, lp_admm_batch, lp_admm_batch_rhs, _, _ = _mods()
    args = dict(admm_instances("sc105", "b_upper"))
    d = load_golden("lp_sc105")
    c, a_eq, beq, a_ineq, bl, bu, lb, ub = solver_args(d)
    args.update(beq=beq, b_lower=bl, b_upper=bu)
    want = lp_admm_batch(args["cs"], a_eq, beq, a_ineq, bl, bu, lb, ub, nb_iter=ITERS)
    got, info = admm_run(args, nb_iter=ITERS)
    assert info is None and np.array_equal(got, want)
    rows = dict(args, beq=np.tile(beq, (ADMM_B, 1)), b_upper=np.tile(bu, (ADMM_B, 1)))
    if bl is not None:
        rows["b_lower"] = np.tile(bl, (ADMM_B, 1))
    got, _ = admm_run(rows, nb_iter=ITERS)
    assert np.array_equal(got, want)
    # the state: identical rows, then 1-D vectors after batched ones, give the state that never called set_rhs
    plain = _mods()[0](args["cs"], a_eq, beq, a_ineq, bl, bu, lb, ub)
    other = _mods()[0](args["cs"], a_eq, 2.0 * beq, a_ineq, bl, bu + 1.0, lb, ub)
    try:
        other.set_rhs(beq=np.tile(3.0 * beq, (ADMM_B, 1)), b_upper=np.tile(bu + 2.0, (ADMM_B, 1)))
        other.set_rhs(beq=beq)
        other.set_rhs(b_upper=bu)
        for st in (plain, other):
            st.iterate(ITERS)
            st.sweep_step()
        assert np.array_equal(plain.x(), other.x()) and np.array_equal(plain.lam(), other.lam())
        assert np.array_equal(plain.report()[:, 1:], other.report()[:, 1:])
    finally:
        plain.close()
        other.close()


def test_admm_set_rhs_after_the_first_iteration_or_half_iteration_is_refused(form):  # noqa: F811
    from pysparselp_amd import SlpError

    args = admm_instances("sc105", "all")
    ref = admm_state_result(args, ITERS)
    for first in ("iterate", "sweep_step"):
        st = admm_state(args)
        try:
            if first == "iterate":
                st.iterate(1)
            else:
                st.sweep_step()
            with pytest.raises(SlpError, match="before the first iteration"):
                st.set_rhs(beq=args["beq"][::-1].copy())
            with pytest.raises(SlpError, match="before the first iteration"):
                st.set_rhs(b_upper=args["b_upper"] + 1.0)
            if first == "sweep_step":
                st.multiplier_step()
            st.iterate(ITERS - 1)
            st.sweep_step()
            assert np.array_equal(st.x(), ref[0]) and np.array_equal(st.lam(), ref[1])   # it runs on with the sides it had
        finally:
            st.close()


def test_solve_admm_batch_rhs_equals_solve_per_instance(form):  # noqa: F811
    """Potts-8, B = 3: with the tolerances of tests/test_gpu_admm_batch.py::test_solve_admm_batch_equals_solve_per_instance."""
    from pysparselp_amd import ORDER_SEQUENTIAL
    from pysparselp_amd.SparseLP import SparseLP

    lp = lp_from_golden(load_golden("lp_potts8"), SparseLP)
    batch, nb_iter = 3, 40
    rs = np.random.RandomState(23)
    costs = np.tile(lp.costsvector, (batch, 1))
    costs[1:] = lp.costsvector * (1 + 0.2 * rs.randn(batch - 1, lp.nb_variables)) + 0.05 * rs.randn(batch - 1, lp.nb_variables)
    sides = dict(b_equalities=perturbed(lp.b_equalities, batch, rs), b_upper=perturbed(lp.b_upper, batch, rs, +1))
    if lp.b_lower is not None and np.size(lp.b_lower):
        sides["b_lower"] = perturbed(lp.b_lower, batch, rs, -1)
    x, elapsed, info = lp.solve_admm_batch_rhs(costs, nb_iter=nb_iter, nb_iter_plot=10, **sides)
    assert x.shape == costs.shape and elapsed > 0 and info is None
    assert lp.itrn_curve == [0, 10, 20, 30, 40]
    for k in range(batch):
        one = copy.deepcopy(lp)
        one.costsvector = costs[k].copy()
        for name, v in sides.items():
            setattr(one, name, v[k].copy())
        xk = one.solve(method="admm", get_timing=False, nb_iter=nb_iter, nb_iter_plot=10, setup="host", order=ORDER_SEQUENTIAL)
        assert np.array_equal(x[k], xk)
        assert one.itrn_curve == lp.itrn_curve
        for name in ("max_violated_equality", "max_violated_inequality", "max_violated_constraint"):
            assert np.array_equal(np.array(getattr(lp, name))[:, k], np.asarray(getattr(one, name), dtype=np.float64)), name
        for name in ("pobj_curve", "dobj_curve"):
            np.testing.assert_allclose(np.array(getattr(lp, name))[:, k], getattr(one, name), **ENERGY_TOL)
    assert all_differ(x)
    out = lp.solve_admm_batch_rhs(costs, tol_residual=1e30, tol_step=1e30, check_every=5, nb_iter=30, get_timing=False, **sides)
    assert out[0].shape == x.shape and out[1]["iterations"].tolist() == [5] * batch and out[1]["stopped"].all()
