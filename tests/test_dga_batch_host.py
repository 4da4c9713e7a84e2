"""Host logic of the batched dual gradient ascent (``dual_gradient_ascent_batch``, ``DeviceDGABatch``,
``SparseLP.solve_dga_batch``): every refusal comes before the library is loaded, and the premise of the GPU parity tests -- on
the batches they use, the device's order of sums gives the reference's iterates -- is checked on the CPU.  None of it needs a GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse

from conftest import REPO, load_golden, lp_from_golden
from dga_batch_cases import BATCH_CASES, STOPS, batch_case, reference_states
from pysparselp_amd import _lib, dual_gradient_ascent_batch
from pysparselp_amd.SparseLP import SparseLP


@pytest.fixture()
def no_library(monkeypatch):
    """Any attempt to load or bind the library fails the test: validation must come first."""
    def refuse(*a, **k):
        raise AssertionError("the library was loaded before the arguments were validated")

    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def _lp(case="sc50a"):
    lp = lp_from_golden(load_golden("lp_" + case), SparseLP)
    return lp, np.tile(lp.costsvector, (3, 1))


def test_shapes_are_refused_before_the_library_is_loaded(no_library):
    lp, costs = _lp()
    n, m_eq, m_in = lp.nb_variables, lp.a_equalities.shape[0], lp.a_inequalities.shape[0]
    assert m_eq > 0 and m_in > 0
    for call in (lambda **k: dual_gradient_ascent_batch(lp, nb_max_iter=5, **k), lambda **k: lp.solve_dga_batch(nb_iter=5, **k)):
        with pytest.raises(ValueError, match="costs has shape"):
            call(costs=costs[0])
        with pytest.raises(ValueError, match="costs has shape"):
            call(costs=costs[:, :-1])
        with pytest.raises(ValueError, match="B >= 1"):
            call(costs=costs[:0])
        with pytest.raises(ValueError, match="lower_bounds has shape"):
            call(costs=costs, lower_bounds=np.zeros((2, n)))
        with pytest.raises(ValueError, match="upper_bounds has shape"):
            call(costs=costs, upper_bounds=np.zeros(n - 1))
    with pytest.raises(ValueError, match="y_eq has shape"):
        dual_gradient_ascent_batch(lp, costs, y_eq=np.zeros((3, m_eq + 1)))
    with pytest.raises(ValueError, match="y_ineq has shape"):
        dual_gradient_ascent_batch(lp, costs, y_ineq=np.zeros((2, m_in)))


@pytest.mark.parametrize("which", ["b_equalities", "b_upper"])
def test_a_right_hand_side_per_instance_is_refused(no_library, which):
    lp, costs = _lp()
    setattr(lp, which, np.tile(getattr(lp, which), (3, 1)))
    with pytest.raises(ValueError, match=which + " has shape .*not built"):
        dual_gradient_ascent_batch(lp, costs)
    with pytest.raises(ValueError, match=which + " has shape .*not built"):
        lp.solve_dga_batch(costs)


@pytest.mark.parametrize("fixture", ["ka_l1svm", "ka_kmedians"])
def test_a_finite_b_lower_is_refused(no_library, fixture):
    lp = lp_from_golden(load_golden(fixture), SparseLP)
    assert lp.b_lower is not None and np.max(lp.b_lower) > -np.inf
    costs = np.tile(lp.costsvector, (2, 1))
    with pytest.raises(ValueError, match="b_lower"):
        dual_gradient_ascent_batch(lp, costs)
    with pytest.raises(ValueError, match="b_lower"):
        lp.solve_dga_batch(costs)


def test_an_lp_without_rows_is_refused(no_library):
    lp, costs = _lp("potts8")
    n = lp.nb_variables
    lp.a_equalities, lp.b_equalities = scipy.sparse.csr_matrix((0, n)), np.zeros(0)
    lp.a_inequalities, lp.b_upper, lp.b_lower = scipy.sparse.csr_matrix((0, n)), np.zeros(0), None
    with pytest.raises(ValueError, match="no constraint rows"):
        dual_gradient_ascent_batch(lp, costs)
    lp.a_inequalities = None
    with pytest.raises(ValueError, match="no constraint rows"):
        dual_gradient_ascent_batch(lp, costs)


def test_an_accepted_batch_gets_as_far_as_the_library(monkeypatch):
    def loaded(*a, **k):
        raise RuntimeError("the library was asked for")

    monkeypatch.setattr(_lib, "load", loaded)
    monkeypatch.setattr(_lib, "lib", loaded)
    lp, costs = _lp()
    with pytest.raises(RuntimeError, match="the library was asked for"):
        dual_gradient_ascent_batch(lp, costs, lower_bounds=np.tile(lp.lower_bounds, (3, 1)))
    with pytest.raises(RuntimeError, match="the library was asked for"):
        lp.solve_dga_batch(costs, nb_iter=5)


def test_solve_batch_still_refuses_dual_gradient_ascent(no_library):
    from pysparselp_amd import SparseLP as module

    lp, costs = _lp("potts8")
    with pytest.raises(ValueError, match="chambolle_pock_ppd"):
        lp.solve_batch(costs, method="dual_gradient_ascent")
    assert module.batch_methods == ("chambolle_pock_ppd",)
    assert module.solving_methods == ("chambolle_pock_ppd", "admm", "admm_blocks", "admm2")
    assert module.dual_methods == ("dual_gradient_ascent",)


def test_signatures():
    e = inspect.Parameter.empty
    params = [(p.name, p.default) for p in inspect.signature(dual_gradient_ascent_batch).parameters.values()]
    assert params == [("lp", e), ("costs", e), ("nb_max_iter", 1000), ("callback_func", None), ("y_eq", None), ("y_ineq", None),
                      ("max_time", None), ("lower_bounds", None), ("upper_bounds", None), ("path", None)]
    params = [(p.name, p.default) for p in inspect.signature(SparseLP.solve_dga_batch).parameters.values()][1:]
    assert params == [("costs", e), ("get_timing", True), ("nb_iter", 10000), ("max_time", None), ("nb_iter_plot", 10),
                      ("ground_truth", None), ("ground_truth_indices", None), ("lower_bounds", None), ("upper_bounds", None)]


def test_status_errors_name_the_instances():
    from pysparselp_amd.DualGradientAscent import STATUS_DRAWS_DRY, STATUS_EMPTY, STATUS_NAN, _check_status_batch

    _check_status_batch(np.zeros(4, dtype=np.int64))
    with pytest.raises(ValueError, match=r"empty breakpoint set.*instances \[1, 3\]"):
        _check_status_batch(np.array([0, STATUS_EMPTY, 0, STATUS_EMPTY]))
    with pytest.raises(ValueError, match=r"NaN.*instances \[2\]"):   # NaN first, as the single solver orders them
        _check_status_batch(np.array([STATUS_EMPTY, 0, STATUS_NAN]))
    _check_status_batch(np.array([STATUS_DRAWS_DRY]) & ~STATUS_DRAWS_DRY)


def test_the_c_abi_is_declared_in_header_binding_and_makefile():
    names = ["create_on", "destroy", "set_path", "path", "sort", "iterate", "iterations", "push_random", "status", "frozen", "get_x", "get_y",
             "report", "timing", "timing_read"]
    assert sorted(n for n in _lib.EXPORTED_SYMBOLS if n.startswith("slp_batch_dga_")) == sorted("slp_batch_dga_" + n for n in names)
    header = open(os.path.join(REPO, "include", "slp_hip.h")).read()
    for name in names:
        assert re.search(r"\bslp_batch_dga_" + name + r"\(", header), name
    csrc = os.path.join(REPO, "pysparselp_amd", "csrc")
    assert "slp_dga_batch.hip" in open(os.path.join(csrc, "Makefile")).read()
    # one copy of the arithmetic: both translation units include the shared header and neither defines its functions again
    for f in ("slp_dga.hip", "slp_dga_batch.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "slp_dga_shared.h"' in text
        for fn in ("key_of", "wave_incl_scan", "group_excl_scan", "tile_values", "alpha_at", "finish_search", "scan_tile_sums"):
            assert not re.search(r"__device__[^;{]*\b" + fn + r"\(", text), (f, fn)


@pytest.mark.parametrize("case", BATCH_CASES)
def test_device_order_gives_the_reference_iterates_on_the_gpu_tests_batches(case):
    """What lets tests/test_gpu_dga_batch.py compare the device with ``order="reference"`` bit for bit: through iteration 100 no
    rounding difference between the two orders of sums lands on a decision, on any of the 24 instances."""
    ref = reference_states(case, "reference")
    dev = reference_states(case, "device")
    _, costs = batch_case(case)
    assert costs.shape[0] == 6 and len(ref) == 6
    for k in range(6):
        assert sorted(ref[k]) == sorted(dev[k]) == [-1] + list(STOPS)
        for it in STOPS:
            for p, q in zip(ref[k][it][:3], dev[k][it][:3]):
                assert (p is None and q is None) or np.array_equal(p, q), (k, it)
            assert ref[k][it][3] == dev[k][it][3], (k, it)
    if case == "potts8":   # the instances stand at different places of the shared stream of draws
        assert len({ref[k][100][3] for k in range(6)}) >= 4


def _same(p, q):
    return all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(p[:3], q[:3])) and p[3] == q[3]


def test_device_order_gives_the_reference_iterates_on_the_tile_remainder_batch():
    from dga_batch_cases import REMAINDER_ITERS, remainder_batch, remainder_states

    _, costs, lbs, ubs = remainder_batch()
    assert costs.shape[0] == 65 and np.count_nonzero(np.any(lbs == ubs, axis=1)) == 13
    ref, dev = remainder_states("reference"), remainder_states("device")
    for k in range(65):
        assert _same(ref[k][REMAINDER_ITERS - 1], dev[k][REMAINDER_ITERS - 1]), k


def test_the_integer_batch_has_several_scan_tiles_and_sums_that_do_not_depend_on_their_order():
    from dga_batch_cases import INT_KEEP, integer_batch, integer_states

    args, costs, lbs, ubs = integer_batch()
    stacked = scipy.sparse.vstack((args[1], args[3])).tocsr()
    counts = {k: [] for k in range(5)}

    def on_search(k, it, kind, direction, c_bar, step, draw):
        a = args[3] if kind == "ineq" else args[1]
        counts[k].append(int(np.count_nonzero(direction * a)))

    ref = integer_states("reference", on_search=on_search)
    dev = integer_states("device")
    for k in range(5):
        for it in INT_KEEP:
            assert _same(ref[k][it], dev[k][it]), (k, it)
    flat = [v for k in counts for v in counts[k]]
    print("breakpoints per search: min", min(flat), "max", max(flat), "per instance", {k: (min(v), max(v)) for k, v in counts.items()})
    # 2 to 5 scan tiles of 1024, a partial last tile, and instances that differ in their number of breakpoints
    assert stacked.shape == (1500, 5000) and min(flat) > 1024 and max(flat) < 5000 and max(flat) > 4096
    assert all(v % 1024 for v in flat) and len({tuple(counts[k]) for k in counts}) == 5
