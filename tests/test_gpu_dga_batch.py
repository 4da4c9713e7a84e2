"""Batched dual gradient ascent on the GPU (csrc/slp_dga_batch.hip): instance k of a batch against tests/dga_cpu.py in the
reference's order of sums (tests/test_dga_batch_host.py checks on the CPU that the device's order gives the same iterates on
these batches), against tests/golden/dga.npz, and against the single-instance ``DeviceDGA`` on instance k's data -- bit for bit,
on both search paths, for batch sizes around the tile of 64 instances, with per-instance bounds, a frozen instance, a shared
stream of tie draws read at per-instance positions, status flags, and through ``SparseLP.solve_dga_batch``."""
import copy
import os

import numpy as np
import pytest
import scipy.sparse

from conftest import Recorder, load_golden, lp_from_golden
from dga_batch_cases import (BATCH_CASES, INT_KEEP, REMAINDER_ITERS, REMAINDER_SIZES, STOPS, batch_case, integer_batch, integer_states,
                             reference_states, remainder_batch, remainder_states)
from dga_cpu import dga_cpu, dual_argmin, dual_energy
from test_dga_host import dga_args
from test_gpu_dga import LP, device_state, start_of

pytestmark = pytest.mark.gpu

# the fused search, and the general one with either of its sorts (one segmented sort / two device-wide stable sorts)
PATHS = ("fused", "general-segmented", "general-global")


def batch_state(args, costs, path, lbs=None, ubs=None):
    """A ``DeviceDGABatch`` over the fixture's rows at the reference's start, its tie draws continuing that stream."""
    from pysparselp_amd.DualGradientAscent import DeviceDGABatch
    from pysparselp_amd.device import DeviceMatrix

    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = args
    y_eq, y_ineq, rs = start_of(a_eq, a_ineq)
    mat = DeviceMatrix.from_blocks(a_eq, a_ineq, c.size)
    b = np.concatenate((b_eq, b_upper if a_ineq is not None else np.zeros(0)))
    path, _, sort = path.partition("-")
    saved = os.environ.get("SLP_DGA_BATCH_SORT")
    if sort:
        os.environ["SLP_DGA_BATCH_SORT"] = sort
    try:
        state = DeviceDGABatch(mat, b, costs, lb if lbs is None else lbs, ub if ubs is None else ubs, np.concatenate((y_eq, y_ineq)),
                               m_eq=a_eq.shape[0], draws=rs.random_sample, path=path)
    finally:
        if sort:
            os.environ.pop("SLP_DGA_BATCH_SORT")
        if saved is not None:
            os.environ["SLP_DGA_BATCH_SORT"] = saved
    assert state.path() == path and state.sort() == (sort or None)
    return state, mat


def test_gpu_dga_batch_small_lps_take_the_fused_search_by_default():
    from pysparselp_amd.DualGradientAscent import DeviceDGABatch
    from pysparselp_amd.device import DeviceMatrix

    args, six = batch_case("potts8")   # n = 176
    y_eq, y_ineq, rs = start_of(args[1], args[3])
    mat = DeviceMatrix.from_blocks(args[1], args[3], args[0].size)
    state = DeviceDGABatch(mat, np.concatenate((args[2], args[4])), six[:2], args[5], args[6], np.concatenate((y_eq, y_ineq)),
                           m_eq=args[1].shape[0], draws=rs.random_sample)
    try:
        assert (state.path(), state.sort()) == ("fused", None)
    finally:
        state.close()
        mat.close()


def snapshot(state):
    flags, draws, _, iters = state.status()
    y_eq, y_ineq = state.y()
    return state.x(), y_eq, y_ineq, draws, flags, iters


def assert_instance(snap, k, ref, what):
    """Instance k of a batch snapshot equals ``ref = (x, y_eq, y_ineq, draws)``."""
    x, y_eq, y_ineq, draws, flags, _ = snap
    assert flags[k] == 0, what
    assert np.array_equal(x[k], ref[0]), what
    assert np.array_equal(y_eq[k], ref[1]), what
    assert np.array_equal(y_ineq[k], ref[2] if ref[2] is not None else np.zeros(0)), what
    assert draws[k] == ref[3], what


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", BATCH_CASES)
def test_gpu_dga_batch_matches_the_reference_instance_by_instance(case, path):
    """Six costs as ONE batch, stopped after 1, 2, 11, 51, 101 iterations (calls of uneven size)."""
    args, costs = batch_case(case)
    ref = reference_states(case)
    g = load_golden("dga")
    golden_it = [int(i) for i in g[f"{case}_it"]]
    state, mat = batch_state(args, costs, path)
    try:
        done = 0
        for it in STOPS:
            state.iterate(it + 1 - done)
            done = it + 1
            snap = snapshot(state)
            assert snap[5] == done
            for k in range(6):
                assert_instance(snap, k, ref[k][it], (case, path, it, k))
            if it in golden_it:   # instance 0 is the fixture's own LP: the reference's recorded iterates
                j = golden_it.index(it)
                assert_instance(snap, 0, (g[f"{case}_x"][j], g[f"{case}_yeq"][j], g[f"{case}_yineq"][j], int(g[f"{case}_draws"][j])),
                                (case, path, it, "golden"))
        assert len(set(snap[3].tolist())) > 1 or case != "potts8"   # the instances stand at different places of the stream
    finally:
        state.close()
        mat.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", BATCH_CASES)
def test_gpu_dga_batch_instance_equals_the_single_solver(case, path):
    """After 101 iterations instance k is the ``DeviceDGA`` run on its data, bit for bit, and so is its report (the reductions
    are shared)."""
    args, costs = batch_case(case)
    state, mat = batch_state(args, costs, path)
    try:
        state.iterate(101)
        snap = snapshot(state)
        report = state.report()
    finally:
        state.close()
        mat.close()
    for k in range(6):
        single, smat = device_state((costs[k],) + tuple(args[1:]), path.partition("-")[0])
        try:
            single.iterate(101)
            flags, draws, _, _ = single.status()
            assert flags == 0
            assert_instance(snap, k, (single.x(), *single.y(), draws), (case, path, k))
            assert tuple(report[k]) == single.report(), (case, path, k)
        finally:
            single.close()
            smat.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("batch", REMAINDER_SIZES)
def test_gpu_dga_batch_sizes_around_the_tile_of_64(batch, path):
    """B = 1, 3, 64, 65 on Potts-8; every fifth instance has a tenth of its variables fixed through per-instance bounds."""
    args, costs, lbs, ubs = remainder_batch()
    ref = remainder_states()
    state, mat = batch_state(args, costs[:batch], path, lbs=lbs[:batch], ubs=ubs[:batch])
    try:
        state.iterate(REMAINDER_ITERS)
        snap = snapshot(state)
        for k in range(batch):
            assert_instance(snap, k, ref[k][REMAINDER_ITERS - 1], (batch, path, k))
    finally:
        state.close()
        mat.close()


@pytest.mark.parametrize("path", PATHS)
def test_gpu_dga_batch_integer_lp_several_scan_tiles_and_a_segmented_sort(path):
    """n = 5000, B = 5: every search has 1289 .. 4671 breakpoints (2 to 5 scan tiles, a partial last one), different per instance;
    instances 3 and 4 have 500 variables fixed."""
    args, costs, lbs, ubs = integer_batch()
    ref = integer_states()
    state, mat = batch_state(args, costs, path, lbs=lbs, ubs=ubs)
    try:
        done = 0
        for it in INT_KEEP:
            state.iterate(it + 1 - done)
            done = it + 1
            snap = snapshot(state)
            for k in range(5):
                assert_instance(snap, k, ref[k][it], (path, it, k))
    finally:
        state.close()
        mat.close()


def _sc50a_with_an_unbounded_instance():
    """SC50A, B = 3; instance 1 has a variable without an upper bound whose reduced cost is negative at the start."""
    args, six = batch_case("sc50a")
    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = args
    costs = six[:3].copy()
    y_eq, y_ineq, _ = start_of(a_eq, a_ineq)
    c_bar = (costs[1] + y_eq * a_eq) + y_ineq * a_ineq
    j = int(np.flatnonzero(c_bar < 0)[0])
    ubs = np.tile(ub, (3, 1))
    ubs[1, j] = np.inf
    assert dual_energy(costs[1], a_eq, b_eq, a_ineq, b_upper, lb, ubs[1], y_eq, y_ineq) == -np.inf
    return args, costs, ubs, j


@pytest.mark.parametrize("path", PATHS)
def test_gpu_dga_batch_a_dual_infeasible_start_freezes_its_instance_only(path):
    args, costs, ubs, j = _sc50a_with_an_unbounded_instance()
    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = args
    y_eq, y_ineq, _ = start_of(a_eq, a_ineq)
    state, mat = batch_state(args, costs, path, ubs=ubs)
    try:
        assert state.frozen().tolist() == [False, True, False]
        state.iterate(50)
        snap = snapshot(state)
        assert state.report()[1, 0] == -np.inf
    finally:
        state.close()
        mat.close()
    start = dga_cpu(costs[1], a_eq, b_eq, a_ineq, b_upper, lb, ubs[1], nb_max_iter=50)
    assert sorted(start) == [-1]
    assert_instance(snap, 1, (start[-1][0], y_eq, y_ineq, 0), "frozen")
    assert snap[0][1, j] == np.inf
    for k in (0, 2):
        single, smat = device_state((costs[k],) + tuple(args[1:]), path.partition("-")[0])
        try:
            single.iterate(50)
            assert_instance(snap, k, (single.x(), *single.y(), single.status()[1]), k)
        finally:
            single.close()
            smat.close()


def test_gpu_dga_batch_function_returns_the_start_of_a_frozen_instance():
    from pysparselp_amd import dual_gradient_ascent_batch
    from pysparselp_amd.DualGradientAscent import dual_gradient_ascent

    args, costs, ubs, j = _sc50a_with_an_unbounded_instance()
    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = args
    x, ye, yi = dual_gradient_ascent_batch(LP(c, a_eq, b_eq, a_ineq, b_upper, lb, ub), costs, nb_max_iter=50, upper_bounds=ubs)
    for k in range(3):
        one = dual_gradient_ascent(None, LP(costs[k], a_eq, b_eq, a_ineq, b_upper, lb, ubs[k]), nb_max_iter=50)
        assert np.array_equal(x[k], one[0]) and np.array_equal(ye[k], one[1]) and np.array_equal(yi[k], one[2]), k


@pytest.mark.parametrize("path", PATHS)
def test_gpu_dga_batch_refills_of_the_shared_draw_buffer_do_not_change_the_result(path):
    args, costs = batch_case("sc50a")
    runs = []
    for chunks in ([120], [1] * 30 + [7] * 10 + [20]):
        state, mat = batch_state(args, costs, path)
        try:
            for k in chunks:
                state.iterate(k)
            snap = snapshot(state)
            assert not snap[4].any() and snap[5] == 120 and snap[3].max() > 0 and len(set(snap[3].tolist())) > 1
            runs.append(snap)
        finally:
            state.close()
            mat.close()
    for p, q in zip(runs[0][:4], runs[1][:4]):
        assert np.array_equal(p, q)
    # a buffer that could run dry stops the call early for the whole batch, sticky bit 4 until the next push
    state, mat = batch_state(args, costs, path)
    try:
        state.push_random(np.random.RandomState(5).random_sample(6))
        state.iterate(10, refill=False)
        flags, _, _, iters = state.status()
        assert np.all(flags & 4) and iters == 3
        state.push_random(np.random.RandomState(6).random_sample(2))
        assert not np.any(state.status()[0] & 4)
    finally:
        state.close()
        mat.close()


@pytest.mark.parametrize("path", PATHS)
def test_gpu_dga_batch_empty_breakpoint_set_sets_the_flag_of_every_instance(monkeypatch, path):
    """The all-zero inequality block of tests/test_gpu_dga.py: the direction meets no column, on every instance."""
    from pysparselp_amd import dual_gradient_ascent_batch
    from pysparselp_amd.DualGradientAscent import STATUS_EMPTY

    args, six = batch_case("sc50a")
    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = args
    empty = scipy.sparse.csr_matrix((np.zeros(6), np.array([0, 5, 1, 7, 2, 9]), np.array([0, 2, 4, 6])), shape=(3, c.size))
    state, mat = batch_state((c, a_eq, b_eq, empty, np.ones(3), lb, ub), six[:3], path)
    try:
        state.iterate(1)
        assert np.all(state.status()[0] & STATUS_EMPTY)
        with pytest.raises(ValueError, match=r"empty breakpoint set.*instances \[0, 1, 2\]"):
            state.check()
    finally:
        state.close()
        mat.close()
    path, _, sort = path.partition("-")
    if sort:
        monkeypatch.setenv("SLP_DGA_BATCH_SORT", sort)
    with pytest.raises(ValueError, match="empty breakpoint set"):
        dual_gradient_ascent_batch(LP(c, a_eq, b_eq, empty, np.ones(3), lb, ub), six[:3], nb_max_iter=5, path=path)


def test_gpu_dga_batch_callbacks_max_time_and_given_multipliers():
    from pysparselp_amd import dual_gradient_ascent_batch
    from pysparselp_amd.DualGradientAscent import dual_gradient_ascent

    args, six = batch_case("sc50a")
    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = args
    lp = LP(c, a_eq, b_eq, a_ineq, b_upper, lb, ub)
    rec = Recorder()
    dual_gradient_ascent_batch(lp, six[:2], nb_max_iter=150, callback_func=rec)
    assert rec.it == [0, 100] and rec.x[0].shape == (2, c.size)
    rec = Recorder()
    out = dual_gradient_ascent_batch(lp, six[:2], nb_max_iter=150, callback_func=rec, max_time=1e-9)   # ends at the first callback
    assert rec.it == [0]
    for k in range(2):
        one = dual_gradient_ascent(None, LP(six[k], a_eq, b_eq, a_ineq, b_upper, lb, ub), nb_max_iter=1)
        assert np.array_equal(out[0][k], one[0]) and np.array_equal(out[1][k], one[1]) and np.array_equal(out[2][k], one[2])
    # the caller's multipliers: shared for y_eq, per instance for y_ineq
    rs = np.random.RandomState(3)
    y_eq, y_ineq = rs.randn(a_eq.shape[0]), rs.rand(2, a_ineq.shape[0])
    out = dual_gradient_ascent_batch(lp, six[:2], nb_max_iter=30, y_eq=y_eq, y_ineq=y_ineq)
    for k in range(2):
        one = dual_gradient_ascent(None, LP(six[k], a_eq, b_eq, a_ineq, b_upper, lb, ub), nb_max_iter=30, y_eq=y_eq, y_ineq=y_ineq[k])
        assert np.array_equal(out[0][k], one[0]) and np.array_equal(out[1][k], one[1]) and np.array_equal(out[2][k], one[2])


@pytest.mark.parametrize("case", ["potts8", "sc50a"])
def test_gpu_solve_dga_batch_curves_solutions_and_certified_bounds(case):
    """B = 3, 201 iterations.  ``dual_lower_bounds[k]`` against ``dga_cpu.dual_energy`` of the returned multipliers: both sum the
    same n terms t_j = min(c_bar_j ub_j, c_bar_j lb_j) (c_bar is the same chain in both) and the same m products y_i b_i, in
    different orders.  A sum of N given terms in any order errs by at most gamma_(N-1) sum|t|, a dot product of m pairs by at
    most gamma_m sum|y_i b_i| (gamma_k = k u / (1 - k u), u = 2^-53); the device adds one subtraction (relative error u), numpy
    two.  The two results therefore differ by at most ((2 n + 1) S_x + (2 m + 3) S_y) u to first order, S_x = sum|t_j|,
    S_y = sum|y_i b_i|, which is below 2 (n + m + 2) u (S_x + S_y) with room for the second-order terms: the constant is 2."""
    from pysparselp_amd.SparseLP import SparseLP

    d = load_golden("lp_" + case)
    lp = lp_from_golden(d, SparseLP)
    args, six = batch_case(case)
    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = args
    costs = six[:3]
    x, elapsed = lp.solve_dga_batch(costs, nb_iter=201, ground_truth=d["gt"], ground_truth_indices=d["gt_idx"])
    assert x.shape == (3, c.size) and elapsed > 0
    assert lp.itrn_curve == [0, 100, 200]
    for name in ("pobj_curve", "dobj_curve", "max_violated_constraint", "max_violated_equality", "max_violated_inequality",
                 "distance_to_ground_truth", "distanceToGroundTruthAfterRounding"):
        curve = getattr(lp, name)
        assert len(curve) == 3 and all(np.shape(v) == (3,) for v in curve), name
    assert len(lp.opttime_curve) == len(lp.dopttime_curve) == 3
    y_eq, y_ineq = lp.dual_multipliers
    assert lp.dual_lower_bounds.shape == (3,) and y_eq.shape == (3, a_eq.shape[0]) and y_ineq.shape == (3, a_ineq.shape[0])
    n, m = c.size, a_eq.shape[0] + a_ineq.shape[0]
    for k in range(3):
        one = copy.deepcopy(lp)
        one.costsvector = costs[k].copy()
        xk = one.solve(method="dual_gradient_ascent", get_timing=False, nb_iter=201, ground_truth=d["gt"], ground_truth_indices=d["gt_idx"])
        assert np.array_equal(x[k], xk), k
        assert one.itrn_curve == lp.itrn_curve
        for name in ("pobj_curve", "dobj_curve", "max_violated_constraint", "distance_to_ground_truth", "distanceToGroundTruthAfterRounding"):
            assert [v[k] for v in getattr(lp, name)] == list(getattr(one, name)), (name, k)
        # the certified bound against the numpy dual energy of the same multipliers
        want = dual_energy(costs[k], a_eq, b_eq, a_ineq, b_upper, lb, ub, y_eq[k], y_ineq[k])
        c_bar, _ = dual_argmin(costs[k], a_eq, a_ineq, lb, ub, y_eq[k], y_ineq[k])
        s_x = np.sum(np.abs(np.minimum(c_bar * ub, c_bar * lb)[c_bar != 0]))
        s_y = np.sum(np.abs(y_eq[k] * b_eq)) + np.sum(np.abs(y_ineq[k] * b_upper))
        bound = 2 * (n + m + 2) * 2.0 ** -53 * (s_x + s_y)
        print(case, k, "dual bound", lp.dual_lower_bounds[k], "numpy", want, "difference", abs(lp.dual_lower_bounds[k] - want), "allowed", bound)
        assert np.isfinite(want) and abs(lp.dual_lower_bounds[k] - want) <= bound, k
    if case == "sc50a":
        # The fixture's solution gt is optimal for c, hence for 2 c.  Weak duality, for any x inside the bounds and any dual
        # feasible y: D(y) <= c.x + y.(K x - b); with gt feasible the last term is <= 0, and it covers gt's residuals exactly.
        gt = d["gt"]
        assert np.all(gt >= lb) and np.all(gt <= ub)
        for k, scale in ((0, 1.0), (1, 2.0)):
            assert np.array_equal(costs[k], scale * c)
            slack = y_eq[k].dot(a_eq * gt - b_eq) + y_ineq[k].dot(a_ineq * gt - b_upper)
            optimum = scale * c.dot(gt)
            print(case, k, "dual bound", lp.dual_lower_bounds[k], "optimal value", optimum, "y.(K gt - b)", slack)
            assert lp.dual_lower_bounds[k] <= optimum + max(slack, 0.0) + 2 * (n + m + 2) * 2.0 ** -53 * (abs(optimum) + abs(slack))


def test_gpu_dga_batch_automatic_path_and_sort():
    """The rule of profiles/dga_batch.json: fused up to 2048 variables and, from 32 instances on, up to 8192; else the general
    search with the global sort."""
    args, costs, lbs, ubs = integer_batch()   # n = 5000
    for batch, path, sort in ((5, "general", "global"), (32, "fused", None)):
        from pysparselp_amd.DualGradientAscent import DeviceDGABatch
        from pysparselp_amd.device import DeviceMatrix

        y_eq, y_ineq, rs = start_of(args[1], args[3])
        mat = DeviceMatrix.from_blocks(args[1], args[3], args[0].size)
        state = DeviceDGABatch(mat, np.concatenate((args[2], args[4])), np.tile(costs, (7, 1))[:batch], args[5], args[6],
                               np.concatenate((y_eq, y_ineq)), m_eq=args[1].shape[0], draws=rs.random_sample)
        try:
            assert (state.path(), state.sort()) == (path, sort), batch
        finally:
            state.close()
            mat.close()
