"""Per-instance stopping of the batched dual gradient ascent on the GPU (csrc/slp_dga_batch.hip, ``DeviceDGABatch.set_stop`` /
``stop_state``, ``dual_gradient_ascent_batch_until``, ``SparseLP.solve_dga_batch_until``).

The yardstick is the batch WITHOUT a test: an unarmed ``DeviceDGABatch`` advanced one iteration at a time, its x, y, tie-draw
counts, flags and ``report()`` read after each -- which gives every instance's step curve (``dga_stop_cpu.steps_of``) and bound
curve -- and, where they cover the case, the iterates of tests/dga_cpu.py.  The expected stopping iterations, reasons and records
come from the restatement tests/dga_batch_stop_cpu.py on those curves, never from the armed run.  Every comparison is exact: the
step is a maximum, the bound a chain of additions shared with the report."""
import functools

import numpy as np
import pytest

import dga_batch_stop_cpu
from conftest import Recorder, load_golden, lp_from_golden
from dga_batch_cases import batch_case, integer_batch, reference_states, remainder_batch
from test_gpu_dga import LP
from test_gpu_dga_batch import PATHS, _sc50a_with_an_unbounded_instance, batch_state, snapshot

pytestmark = pytest.mark.gpu

inf = np.inf
TOTAL, EVERY = 200, 10          # the sc50a batch: horizon and cadence
R_TOTAL = 21                    # Potts-8 around the tile of 64
I_TOTAL = 30                    # the integer LP


def case_of(name):
    """``(args, costs, lbs, ubs)`` of a named batch."""
    if name == "sc50a":
        return batch_case("sc50a") + (None, None)
    if name == "remainder":
        return remainder_batch()
    if name == "integer":
        return integer_batch()
    if name == "unbounded":
        args, costs, ubs, _ = _sc50a_with_an_unbounded_instance()
        return args, costs, None, ubs
    raise KeyError(name)


def armed(name, path, batch=None):
    args, costs, lbs, ubs = case_of(name)
    cut = slice(0, batch)
    return batch_state(args, costs[cut], path, lbs=None if lbs is None else lbs[cut], ubs=None if ubs is None else ubs[cut])


@functools.lru_cache(maxsize=None)
def baseline(name, path, total):
    """The unarmed batch one iteration at a time: ``snaps[t]`` = ``(x, y_eq, y_ineq, draws, flags, iterations)`` after ``t``
    iterations, ``steps[k][t - 1]`` and ``bounds[k][t - 1]`` the curves of instance ``k``, ``frozen``.  Shared, never modified."""
    state, mat = armed(name, path)
    try:
        frozen = state.frozen()
        snaps, reports = [snapshot(state)], [state.report()[:, 0]]
        for _ in range(total):
            state.iterate(1)
            snaps.append(snapshot(state))
            reports.append(state.report()[:, 0])
        assert snaps[-1][5] == total
    finally:
        state.close()
        mat.close()
    batch = snaps[0][0].shape[0]
    steps = np.zeros((batch, total))
    for k in range(batch):
        if frozen[k]:
            continue
        states = {t - 1: (None, snaps[t][1][k], snaps[t][2][k], 0) for t in range(total + 1)}
        steps[k] = dga_batch_stop_cpu.steps_of(states)
    bounds = np.array(reports[1:]).T.copy()
    for a in (steps, bounds):
        a.setflags(write=False)
    return dict(snaps=snaps, steps=steps, bounds=bounds, frozen=frozen)


def expected(base, rules, total, batch=None):
    cut = slice(0, batch)
    return dga_batch_stop_cpu.stop_state(base["steps"][cut], base["bounds"][cut], rules, total, frozen=base["frozen"][cut])


def assert_state(state, base, want, what):
    """The armed ``state`` reports ``want`` (the restatement's stop state) and every instance stands, bit for bit, where the
    unarmed batch stood after that instance's iterations; a stopped instance's bound is the report's."""
    got = state.stop_state()
    assert got[0].dtype == np.int64 and got[1].dtype == bool and got[4].dtype == np.int32, what
    print(what, "iterations", got[0].tolist(), "reason", got[4].tolist(), "want", want[0].tolist(), want[4].tolist())
    for g, w, label in zip(got, want, ("iterations", "stopped", "step", "bound", "reason")):
        assert np.array_equal(g, w, equal_nan=True), (what, label, g, w)
    x, y_eq, y_ineq, draws, flags, _ = snapshot(state)
    report = state.report()[:, 0]
    frozen = state.frozen()
    assert np.array_equal(frozen, base["frozen"][:frozen.size]), what   # "frozen" keeps meaning a dual-infeasible start
    for k, t in enumerate(want[0]):
        ref = base["snaps"][int(t)]
        assert np.array_equal(x[k], ref[0][k]), (what, k, "x")
        assert np.array_equal(y_eq[k], ref[1][k]) and np.array_equal(y_ineq[k], ref[2][k]), (what, k, "y")
        assert draws[k] == ref[3][k] and flags[k] == ref[4][k], (what, k, "draws, flags")
        if t > 0:
            assert report[k] == base["bounds"][k][int(t) - 1], (what, k, "report")
        if want[1][k] and want[4][k] & 2:
            assert got[3][k] == report[k], (what, k, "bound")


def sc50a_rule(base):
    """``(tol, targets)`` chosen on the unarmed curves so that two instances stop by their step, two more by a cut-off taken from
    their own bound curve at the middle check, and two never stop within the horizon (one with ``+inf``, one with a cut-off above
    every bound).  The mix is asserted on the restatement, so a wrong choice fails here."""
    steps, bounds = base["steps"], base["bounds"]
    least = steps[:, EVERY - 1::EVERY].min(axis=1)       # the smallest step an instance shows at a check
    order = np.argsort(least, kind="stable")
    tol = float(least[order[1]])
    targets = np.full(6, inf)
    middle = TOTAL // 2
    for k in order[2:4]:
        targets[k] = bounds[k][middle - 1]
    targets[order[5]] = bounds.max() + 1.0
    want = dga_batch_stop_cpu.stop_state(steps, bounds, [(0, tol, targets, EVERY)], TOTAL)
    reason = want[4]
    assert np.sum(reason & 1 > 0) >= 2 and np.sum(reason & 2 > 0) >= 2 and np.sum(reason == 0) >= 2, (tol, targets, want)
    assert len(set(want[0][want[1]].tolist())) > 1 and want[0][want[1]].max() < TOTAL, want
    return tol, targets


@pytest.mark.parametrize("path", PATHS)
def test_gpu_dga_batch_stop_sc50a_step_bound_and_never(path):
    base = baseline("sc50a", path, TOTAL)
    assert not base["frozen"].any()
    # the unarmed batch is the reference's iterates where tests/dga_cpu.py recorded them
    ref = reference_states("sc50a")
    for k in range(6):
        for it in (0, 10, 100):
            assert np.array_equal(base["snaps"][it + 1][0][k], ref[k][it][0]) and np.array_equal(base["snaps"][it + 1][1][k], ref[k][it][1])
    tol, targets = sc50a_rule(base)
    want = expected(base, [(0, tol, targets, EVERY)], TOTAL)
    state, mat = armed("sc50a", path)
    try:
        got = state.stop_state()   # before arming: nothing evaluated
        assert not got[0].any() and not got[1].any() and np.all(got[2] == inf) and np.all(got[3] == -inf) and not got[4].any()
        state.set_stop(tol, targets, EVERY)
        state.iterate(TOTAL)
        assert state.status()[3] == TOTAL
        assert_state(state, base, want, ("sc50a", path))
    finally:
        state.close()
        mat.close()


@pytest.mark.parametrize("every", (1, 7))
@pytest.mark.parametrize("batch", (1, 3, 64, 65))
@pytest.mark.parametrize("path", ("fused", "general-segmented"))
def test_gpu_dga_batch_stop_sizes_around_the_tile_of_64(path, batch, every):
    """Potts-8 with per-instance bounds; every second instance has a cut-off from its own bound curve, the step tolerance is the
    median of the smallest steps the instances show at a check."""
    base = baseline("remainder", path, R_TOTAL)
    steps, bounds = base["steps"][:batch], base["bounds"][:batch]
    tol = float(np.median(steps[:, every - 1::every].min(axis=1)))
    targets = np.full(batch, inf)
    middle = max(every, R_TOTAL // 2 // every * every)   # a check near the middle of the run
    targets[::2] = bounds[::2, middle - 1]
    want = expected(base, [(0, tol, targets, every)], R_TOTAL, batch)
    assert want[1].any(), want
    state, mat = armed("remainder", path, batch)
    try:
        state.set_stop(tol, targets, every)
        state.iterate(R_TOTAL)
        assert_state(state, base, want, ("remainder", path, batch, every))
    finally:
        state.close()
        mat.close()


@pytest.mark.parametrize("path", ("general-segmented", "general-global"))
def test_gpu_dga_batch_stop_integer_lp_empty_segments_between_live_ones(path):
    """n = 5000, B = 5, the general search: instances 1 and 3 are retired early by their cut-offs, so their sort segments are
    empty between live ones; the others stay bit for bit."""
    base = baseline("integer", path, I_TOTAL)
    targets = np.full(5, inf)
    targets[1], targets[3] = base["bounds"][1][4], base["bounds"][3][9]
    want = expected(base, [(0, None, targets, 5)], I_TOTAL)
    assert want[1].tolist() == [False, True, False, True, False] and want[0][1] <= 5 and want[0][3] <= 10, want
    state, mat = armed("integer", path)
    try:
        state.set_stop(None, targets, 5)
        state.iterate(I_TOTAL)
        assert_state(state, base, want, ("integer", path))
    finally:
        state.close()
        mat.close()


@pytest.mark.parametrize("path", ("fused", "general-global"))
def test_gpu_dga_batch_stop_a_frozen_instance_stays_frozen_and_is_never_stopped(path, monkeypatch):
    from pysparselp_amd import dual_gradient_ascent_batch_until

    base = baseline("unbounded", path, 30)
    assert base["frozen"].tolist() == [False, True, False]
    tol = float(base["steps"][[0, 2], 9::10].max()) * 2.0   # both moving instances meet it at the first check
    want = expected(base, [(0, tol, None, 10)], 30)
    assert want[0].tolist() == [10, 0, 10] and want[1].tolist() == [True, False, True]
    state, mat = armed("unbounded", path)
    try:
        state.set_stop(tol, None, 10)
        state.iterate(30)
        assert state.status()[3] == 30    # nothing is read back inside a call: it launched its thirty iterations ...
        state.iterate(5)
        assert state.status()[3] == 30    # ... and the next one, which finds nothing moving, launches nothing
        assert_state(state, base, want, ("unbounded", path))
    finally:
        state.close()
        mat.close()
    # the function: the run ends when the others have stopped
    args, costs, _, ubs = case_of("unbounded")
    p, _, sort = path.partition("-")
    if sort:
        monkeypatch.setenv("SLP_DGA_BATCH_SORT", sort)
    rec = Recorder()
    x, y_eq, y_ineq, info = dual_gradient_ascent_batch_until(LP(*args), costs, tol, None, 10, nb_max_iter=500, callback_func=rec,
                                                             upper_bounds=ubs, path=p)
    assert rec.it == [0]
    assert info["iterations"].tolist() == [10, 0, 10] and info["stopped"].tolist() == [True, False, True]
    assert info["reason"].tolist() == [1, 0, 1] and info["lower_bound"][1] == -inf
    for k, t in enumerate((10, 0, 10)):
        assert np.array_equal(x[k], base["snaps"][t][0][k]) and np.array_equal(y_eq[k], base["snaps"][t][1][k]), k
        assert np.array_equal(y_ineq[k], base["snaps"][t][2][k]), k


@pytest.mark.parametrize("path", ("fused", "general-segmented"))
def test_gpu_dga_batch_stop_does_not_depend_on_how_the_run_is_split_nor_on_refills(path):
    """Calls of uneven size, then one iteration per call -- every call tops the draw buffer up and drops what every MOVING
    instance has passed, behind the stopped ones -- and draws pushed by hand behind the stopped instances."""
    base = baseline("sc50a", path, TOTAL)
    tol, targets = sc50a_rule(base)
    want = expected(base, [(0, tol, targets, EVERY)], TOTAL)
    first = int(want[0][want[1]].min())
    for chunks in ((1, 2, 11, 51, 135), (first,) + (1,) * (TOTAL - first), (first, 0, TOTAL - first)):
        assert sum(chunks) == TOTAL
        state, mat = armed("sc50a", path)
        try:
            state.set_stop(tol, targets, EVERY)
            for j, k in enumerate(chunks):
                if k == 0:   # a forced refill: the stream goes on, the front of the window moves past the stopped instances
                    before = state.status()
                    state.push_random(state._draws(64))
                    after = state.status()
                    assert after[2] == before[2] + 64 and np.array_equal(after[1], before[1])
                    continue
                state.iterate(k)
                assert state.status()[3] == sum(chunks[:j + 1])
            assert_state(state, base, want, ("split", path, chunks[:4]))
        finally:
            state.close()
            mat.close()


def test_gpu_dga_batch_stop_armed_at_iteration_7_counts_the_cadence_over_the_life_of_the_state():
    base = baseline("sc50a", "fused", TOTAL)
    tol, targets = sc50a_rule(base)
    rules = [(7, tol, targets, 5)]
    want = expected(base, rules, TOTAL)
    assert want[1].any() and np.all(want[0][want[1]] % 5 == 0)
    state, mat = armed("sc50a", "fused")
    try:
        state.iterate(7)
        state.set_stop(tol, targets, 5)
        state.iterate(2)
        assert_state(state, base, expected(base, rules, 9), "armed at 7, after 9")   # nothing evaluated yet
        state.iterate(TOTAL - 9)
        assert_state(state, base, want, "armed at 7")
    finally:
        state.close()
        mat.close()


def test_gpu_dga_batch_stop_a_stopped_instance_is_not_restarted():
    """Re-armed with a tighter rule, a looser one, and turned off: the stopped instances keep their records, the rule applies to
    the instances still moving."""
    base = baseline("sc50a", "fused", TOTAL)
    tol, targets = sc50a_rule(base)
    huge = float(base["steps"].max()) * 2.0
    for label, second in (("tighter", (100, 0.0, None, 1)), ("looser", (100, huge, None, EVERY)), ("off", (100, None, None, 1))):
        rules = [(0, tol, targets, EVERY), second]
        at_100, want = expected(base, rules[:1], 100), expected(base, rules, TOTAL)
        assert at_100[1].any() and not at_100[1].all()
        assert np.array_equal(want[0][at_100[1]], at_100[0][at_100[1]])
        if label == "looser":
            assert want[1].all() and np.all(want[0][~at_100[1]] == 100 + EVERY)
        state, mat = armed("sc50a", "fused")
        try:
            state.set_stop(tol, targets, EVERY)
            state.iterate(100)
            assert_state(state, base, at_100, (label, 100))
            state.set_stop(*second[1:])
            state.iterate(TOTAL - 100)
            assert state.status()[3] == TOTAL
            if label == "looser":   # everything is stopped: a further call launches nothing, the count and every array stay
                held = snapshot(state), state.report(), state.stop_state()
                state.iterate(100)
                assert state.status()[3] == TOTAL
                for p, q in zip(held[0] + (held[1],) + held[2], snapshot(state) + (state.report(),) + state.stop_state()):
                    assert np.array_equal(p, q, equal_nan=True)
            assert_state(state, base, want, (label, TOTAL))
        finally:
            state.close()
            mat.close()


@pytest.mark.parametrize("path", PATHS)
def test_gpu_dga_batch_until_end_to_end(path, monkeypatch):
    from pysparselp_amd import dual_gradient_ascent_batch, dual_gradient_ascent_batch_until
    from pysparselp_amd.SparseLP import SparseLP

    base = baseline("sc50a", path, TOTAL)
    tol, targets = sc50a_rule(base)
    huge = float(base["steps"][:, EVERY - 1::EVERY].max()) * 2.0
    args, costs = batch_case("sc50a")
    p, _, sort = path.partition("-")
    if sort:
        monkeypatch.setenv("SLP_DGA_BATCH_SORT", sort)
    seen = []

    def callback(niter, x, *rest):
        info = callback.info
        seen.append((niter, info["iterations"].copy(), info["stopped"].copy(), x.copy()))

    x, y_eq, y_ineq, info = dual_gradient_ascent_batch_until(LP(*args), costs, tol, targets, EVERY, nb_max_iter=TOTAL, callback_func=callback,
                                                             path=p)
    want = expected(base, [(0, tol, targets, EVERY)], TOTAL)
    assert sorted(info) == ["iterations", "lower_bound", "reason", "step", "stopped"]
    for name, w in zip(("iterations", "stopped", "step", None, "reason"), want):
        if name:
            assert np.array_equal(info[name], w, equal_nan=True), name
    for k, t in enumerate(want[0]):
        ref = base["snaps"][int(t)]
        assert np.array_equal(x[k], ref[0][k]) and np.array_equal(y_eq[k], ref[1][k]) and np.array_equal(y_ineq[k], ref[2][k]), k
        assert info["lower_bound"][k] == base["bounds"][k][int(t) - 1], k     # the final report
    # info is current at every callback: after 1 and after 101 iterations
    assert [s[0] for s in seen] == [0, 100]
    for niter, iterations, stopped, xs in seen:
        at = expected(base, [(0, tol, targets, EVERY)], niter + 1)
        assert np.array_equal(iterations, at[0]) and np.array_equal(stopped, at[1]), niter
        for k, t in enumerate(at[0]):
            assert np.array_equal(xs[k], base["snaps"][int(t)][0][k]), (niter, k)
    # a rule every instance meets at the first check ends the run long before nb_max_iter
    rec = Recorder()
    out = dual_gradient_ascent_batch_until(LP(*args), costs, huge, None, EVERY, nb_max_iter=5000, callback_func=rec, path=p)
    assert rec.it == [0] and np.all(out[3]["iterations"] == EVERY) and out[3]["stopped"].all() and np.all(out[3]["reason"] == 1)
    assert np.array_equal(out[0], base["snaps"][EVERY][0])
    # SparseLP
    d = load_golden("lp_sc50a")
    lp = lp_from_golden(d, SparseLP)
    xs, elapsed = lp.solve_dga_batch_until(costs, tol, targets, EVERY, nb_iter=TOTAL, ground_truth=d["gt"], ground_truth_indices=d["gt_idx"])
    assert elapsed > 0 and np.array_equal(xs, x)
    assert lp.itrn_curve == [0, 100] and all(np.shape(v) == (6,) for v in lp.dobj_curve) and len(lp.pobj_curve) == 2
    assert np.array_equal(lp.dual_multipliers[0], y_eq) and np.array_equal(lp.dual_multipliers[1], y_ineq)
    assert np.array_equal(lp.dual_lower_bounds, info["lower_bound"])
    for name in info:
        assert np.array_equal(lp.stop_info[name], info[name], equal_nan=True), name
    # the function without a test returns what it returned before: the reference's iterates, the recorded ones for instance 0
    plain = dual_gradient_ascent_batch(LP(*args), costs, nb_max_iter=101, path=p)
    ref = reference_states("sc50a")
    g = load_golden("dga")
    j = [int(i) for i in g["sc50a_it"]].index(100)
    for k in range(6):
        assert np.array_equal(plain[0][k], ref[k][100][0]) and np.array_equal(plain[1][k], ref[k][100][1]), k
        assert np.array_equal(plain[2][k], ref[k][100][2]), k
    assert np.array_equal(plain[0][0], g["sc50a_x"][j]) and np.array_equal(plain[1][0], g["sc50a_yeq"][j])
    assert np.array_equal(plain[2][0], g["sc50a_yineq"][j])
