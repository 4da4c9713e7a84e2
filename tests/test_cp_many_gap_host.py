"""Host side of the certificate the Chambolle-Pock list solver can stop on (``CPManyState.set_stop_gap`` / ``gap_state``,
``chambolle_pock_ppd_many_certified``, ``solve_many_certified``): the refusals come before the library is touched, the two new
prototypes are declared and bound, and the lists of tests/test_gpu_cp_many_gap.py have what makes them a test -- every check
decidable, stops spread over the run, LPs that do not stop -- conditions on the inputs, derived from the numpy restatement
(tests/cp_gap_cpu.py) alone.  None of it needs a GPU."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse

import cp_gap_cpu
import pysparselp_amd
from conftest import REPO, load_golden, lp_from_golden
from pysparselp_amd import _lib, chambolle_pock_ppd_many_certified, solve_many_certified
from pysparselp_amd.ChambollePockPPD import CPManyState
from pysparselp_amd.SparseLP import SparseLP
from test_cp_many_stop_host import BAD_EVERY, BAD_TOL, CASES, ITERATIONS, _problems, no_library  # noqa: F401
from test_oracle_golden import _reduced

TOL_GAP = TOL_FEAS = 1e-2
EVERY = (1, 4, 10)
RANDOM_SEED, RANDOM_COUNT, RANDOM_ITERATIONS, RANDOM_EVERY, RANDOM_LEFT_OUT = 7, 24, 300, 3, 2


@functools.lru_cache(maxsize=None)
def fixture_certificates(case, nb_iter=ITERATIONS):
    """The restatement's certificates of a reduced golden LP for ``t = 1 .. nb_iter`` (shared, read only)."""
    problem = _reduced(load_golden("lp_" + case))
    return cp_gap_cpu.certificates(problem, *cp_gap_cpu.iterates(problem, nb_iter))


@functools.lru_cache(maxsize=None)
def random_problems():
    return tuple(cp_gap_cpu.random_list(RANDOM_SEED, RANDOM_COUNT))


@functools.lru_cache(maxsize=None)
def random_certificates():
    """Per LP of the seeded list: its certificates over ``RANDOM_ITERATIONS`` iterations (shared, read only)."""
    return tuple(cp_gap_cpu.certificates(p, *cp_gap_cpu.iterates(p, RANDOM_ITERATIONS)) for p in random_problems())


def random_left_out():
    """The LPs of the seeded list with an undecidable check: no part in the comparison of stopping iterations."""
    return [k for k, cert in enumerate(random_certificates())
            if not cp_gap_cpu.all_decidable(cert, TOL_GAP, TOL_FEAS, RANDOM_EVERY, RANDOM_ITERATIONS)]


class _NoState(CPManyState):
    """A state without a device: ``set_stop_gap`` must refuse before it looks for one."""

    def __init__(self):
        pass

    def close(self):
        pass

    __del__ = close


def test_a_bad_tolerance_or_cadence_is_refused_before_the_library(no_library):  # noqa: F811
    ps = _problems()
    lps = [lp_from_golden(load_golden("lp_potts8"), SparseLP)]
    st = _NoState()
    for tol in BAD_TOL:
        for name, args in (("tol_gap", (tol, 1e-2)), ("tol_feas", (1e-2, tol))):
            match = f"{name} must be a finite float >= 0"
            with pytest.raises(ValueError, match=match):
                chambolle_pock_ppd_many_certified(ps, *args)
            with pytest.raises(ValueError, match=match):
                solve_many_certified(lps, *args)
            if not (name == "tol_gap" and tol is None):   # None is how the state's test is turned off
                with pytest.raises(ValueError, match=match):
                    st.set_stop_gap(*args)
    for every in BAD_EVERY:
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            chambolle_pock_ppd_many_certified(ps, 1e-2, 1e-2, every)
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            solve_many_certified(lps, 1e-2, 1e-2, check_every=every)
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            st.set_stop_gap(1e-2, 1e-2, every)
    with pytest.raises(ValueError, match="empty list"):
        chambolle_pock_ppd_many_certified([], 1e-2, 1e-2)
    with pytest.raises(ValueError, match="LP 1 is not a tuple of 8"):
        chambolle_pock_ppd_many_certified([ps[0], ps[1][:7]], 1e-2, 1e-2)
    with pytest.raises(ValueError, match="empty list"):
        solve_many_certified([], 1e-2, 1e-2)


def test_an_accepted_call_gets_as_far_as_the_library(no_library):  # noqa: F811
    with pytest.raises(AssertionError, match="library was loaded"):
        chambolle_pock_ppd_many_certified(_problems(), 0.0, 0.0, 1, nb_max_iter=3)
    with pytest.raises(AssertionError, match="library was loaded"):
        solve_many_certified([lp_from_golden(load_golden("lp_potts8"), SparseLP)], 1e-2, 1e-2, nb_iter=3)


def test_lps_without_rows_are_stopped_after_no_iteration(no_library):  # noqa: F811
    rng = np.random.RandomState(5)
    ps = []
    for n in (4, 1):
        c = rng.randn(n)
        ps.append((c, None, None, scipy.sparse.csr_matrix((0, n)), None, np.zeros(0), -rng.rand(n) - 1, rng.rand(n) + 1))
    xs, best, info = chambolle_pock_ppd_many_certified(ps, 1e-2, 1e-2)
    assert best == [None, None]
    assert sorted(info) == ["iterations", "lower_bound", "primal", "stopped", "violation"]
    assert info["iterations"].dtype == np.int64 and info["stopped"].dtype == bool
    assert all(info[name].dtype == np.float64 for name in ("primal", "lower_bound", "violation"))
    assert np.array_equal(info["iterations"], [0, 0]) and np.array_equal(info["stopped"], [True, True])
    for k, ((c, *_, lb, ub), x) in enumerate(zip(ps, xs)):
        assert np.array_equal(x, np.where(c > 0, lb, np.where(c < 0, ub, 0.0)))
        assert info["primal"][k] == info["lower_bound"][k] == c.dot(x) and info["violation"][k] == 0.0


def test_names_and_signatures():
    for name in ("chambolle_pock_ppd_many_certified", "solve_many_certified"):
        assert name in pysparselp_amd.__all__ and hasattr(pysparselp_amd, name), name
    assert str(inspect.signature(chambolle_pock_ppd_many_certified)) == (
        "(problems, tol_gap, tol_feas, check_every=10, x0=None, alpha=1, theta=1, nb_max_iter=10000, callback_func=None, "
        "max_time=None, nb_iter_plot=10)")
    assert str(inspect.signature(solve_many_certified)) == (
        "(lps, tol_gap, tol_feas, check_every=10, get_timing=True, nb_iter=10000, max_time=None, nb_iter_plot=10)")
    assert pysparselp_amd.SparseLP.solve_many_certified is solve_many_certified
    assert str(inspect.signature(CPManyState.set_stop_gap)) == "(self, tol_gap, tol_feas, check_every=1)"
    assert str(inspect.signature(CPManyState.gap_state)) == "(self)"
    assert "fixed_cost" in solve_many_certified.__doc__ and "remove_fixed_variables" in solve_many_certified.__doc__


def test_the_two_prototypes_are_declared_and_bound():
    text = open(os.path.join(REPO, "include", "slp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"\s+", " ", text)
    assert "int slp_many_cpgap_set_stop(slp_cp_many *s, double tol_gap, double tol_feas, int64_t check_every);" in text
    assert ("int slp_many_cpgap_state(slp_cp_many *s, int64_t *iterations, int32_t *stopped, double *primal, double *bound, "
            "double *violation);") in text
    lib = _lib.load()   # dlopen works without a GPU
    for name in ("slp_many_cpgap_set_stop", "slp_many_cpgap_state"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.slp_many_cpgap_set_stop.argtypes == [_lib.c_vp, _lib.c_dbl, _lib.c_dbl, _lib.c_i64]
    assert lib.slp_many_cpgap_state.argtypes == [_lib.c_vp] * 6
    assert len(_lib.EXPORTED_SYMBOLS) == 215
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "C ABI (215 entry points)" in readme


def test_the_restatement_on_a_hand_made_lp():
    """min x0 + 2 x1, x0 + x1 = 1, x0 - x1 <= 0.5, 0 <= x <= 1 (x1 free below in the second LP)."""
    a_eq, a_in = scipy.sparse.csr_matrix([[1.0, 1.0]]), scipy.sparse.csr_matrix([[1.0, -1.0]])
    p = (np.array([1.0, 2.0]), a_eq, np.array([1.0]), a_in, None, np.array([0.5]), np.zeros(2), np.ones(2))
    r = cp_gap_cpu.Restatement(p)
    x, y = np.array([0.75, 0.25]), np.array([-1.5, 0.5])    # d = c + K^T y = (1 - 1.5 + 0.5, 2 - 1.5 - 0.5) = (0, 0)
    cert = r.at(x, y)
    assert cert.primal == 1.25 and cert.bound == 0.0 - (-1.5 * 1.0 + 0.5 * 0.5) and cert.violation == 0.0
    assert cp_gap_cpu.decision(cert.primal, cert.bound, cert.violation, 0.0, 0.0)   # optimal: gap 0
    cert = r.at(np.array([1.0, 0.25]), np.array([-1.0, 0.0]))   # d = (0, 1): term min(0, 1) = 0; K x - b = (0.25, 0.25)
    assert cert.primal == 1.5 and cert.bound == 1.0 and cert.violation == 0.25
    assert not cp_gap_cpu.decision(cert.primal, cert.bound, cert.violation, 1.0, 0.2)
    assert cp_gap_cpu.decision(cert.primal, cert.bound, cert.violation, 0.15, 0.25)   # 0.5 <= 0.15 * 3.5
    free = p[:6] + (np.array([0.0, -np.inf]), np.ones(2))
    cert = cp_gap_cpu.Restatement(free).at(np.array([1.0, 0.25]), np.array([-1.0, 0.0]))   # d_1 = 1 > 0 on a variable free below
    assert cert.bound == -np.inf and not cp_gap_cpu.decision(cert.primal, cert.bound, cert.violation, 1e9, 1e9)
    nan = (np.array([1.0, np.nan]),) + p[1:]
    cert = cp_gap_cpu.Restatement(nan).at(x, y)
    assert np.isnan(cert.primal) and not cp_gap_cpu.decision(cert.primal, cert.bound, cert.violation, 1e9, 1e9)
    no_side = p[:5] + (np.array([np.inf]),) + p[6:]    # a row without a finite side: y = 0 keeps 0 * inf out
    cert = cp_gap_cpu.Restatement(no_side).at(x, np.array([-1.5, 0.0]))
    assert np.isfinite(cert.bound) and cert.violation == 0.0
    # the state a run reports
    cert = cp_gap_cpu.Certificate(*(np.array(v) for v in ([3.0, 2.0, 1.5, 1.0], [0.0, 0.5, 1.0, 1.0], [0.5, 0.0, 0.0, 0.0], [0.0] * 4)))
    assert cp_gap_cpu.stopping_iteration(cert, 0.2, 0.1, 1) == 3 and cp_gap_cpu.stopping_iteration(cert, 0.2, 0.1, 2) == 4
    assert cp_gap_cpu.stopping_iteration(cert, 0.2, 0.1, 1, after=3) == 4
    assert cp_gap_cpu.gap_state(cert, 0.2, 0.1, 1, 4) == (3, True, 1.5, 1.0, 0.0)
    assert cp_gap_cpu.gap_state(cert, 0.0, 0.1, 2, 3) == (3, False, 2.0, 0.5, 0.0)
    assert cp_gap_cpu.gap_state(cert, 0.0, 0.1, 3, 2) == (2, False, np.inf, -np.inf, np.inf)


def _assert_list_condition(stops, bands, count_ok):
    print("first stops", stops)
    print("fewest bands from a threshold", {k: f"{v:.3g}" for k, v in bands.items()})
    reached = [t for t in stops.values() if t is not None]
    assert len(reached) >= 4 and len(set(reached)) >= 4, stops
    assert count_ok


@pytest.mark.parametrize("every", EVERY)
def test_the_fixture_list_is_decidable_and_spreads_its_stops(every):
    """What makes the GPU cases a test, at ``tol_gap = tol_feas = 1e-2`` over 200 iterations: every check of every LP is decidable, at
    least four LPs stop, at pairwise different iterations, and sc50a and sc105 -- which the step test stops or would stop at a gap
    of 0.99 -- do not."""
    stops, bands = {}, {}
    for c in CASES:
        cert = fixture_certificates(c)
        stops[c] = cp_gap_cpu.stopping_iteration(cert, TOL_GAP, TOL_FEAS, every)
        evaluated = cp_gap_cpu.checks(ITERATIONS if stops[c] is None else stops[c], every)
        bands[c] = min(cp_gap_cpu.bands_from_threshold(cert, t, TOL_GAP, TOL_FEAS) for t in evaluated)
        assert cp_gap_cpu.all_decidable(cert, TOL_GAP, TOL_FEAS, every, ITERATIONS), c
        assert stops[c] is None or (stops[c] % every == 0 and 1 < stops[c] < ITERATIONS)
    reached = [stops[c] for c in CASES if stops[c] is not None]
    _assert_list_condition(stops, bands, len(reached) == len(set(reached)) == 4)
    assert stops["sc50a"] is None and stops["sc105"] is None
    last = fixture_certificates("sc105")
    gap = abs(last.primal[-1] - last.bound[-1]) / (1 + abs(last.primal[-1]) + abs(last.bound[-1]))
    assert gap > 0.9   # where the step test at 1e-2 has long stopped it (tests/test_gpu_cp_many_stop.py)


def test_the_seeded_random_list_stays_within_its_cap():
    left_out = random_left_out()
    print("left out", left_out)
    assert len(left_out) <= RANDOM_LEFT_OUT
    problems, certs = random_problems(), random_certificates()
    assert len(problems) == RANDOM_COUNT
    stops, bands = {}, {}
    for k, cert in enumerate(certs):
        if k in left_out:
            continue
        stops[k] = cp_gap_cpu.stopping_iteration(cert, TOL_GAP, TOL_FEAS, RANDOM_EVERY)
        evaluated = cp_gap_cpu.checks(RANDOM_ITERATIONS if stops[k] is None else stops[k], RANDOM_EVERY)
        bands[k] = min(cp_gap_cpu.bands_from_threshold(cert, t, TOL_GAP, TOL_FEAS) for t in evaluated)
    _assert_list_condition(stops, bands, any(t is None for t in stops.values()))
    # the shapes the list is there for
    shapes = [(p[0].size, 0 if p[1] is None else p[1].shape[0], 0 if p[3] is None else p[3].shape[0]) for p in problems]
    assert all(1 <= n <= 40 and 1 <= me + mi <= 40 for n, me, mi in shapes), shapes
    assert any(n == 1 for n, _, _ in shapes) and any(me + mi == 1 for _, me, mi in shapes)
    assert any(mi == 0 for _, _, mi in shapes) and any(me == 0 for _, me, _ in shapes) and any(me and mi for _, me, mi in shapes)
    assert any(np.isinf(p[6]).any() or np.isinf(p[7]).any() for p in problems)
    assert any(np.isneginf(cert.bound).any() for cert in certs)
