"""Compaction for the ADMM list solver (csrc/slp_admm_many.hip: ``ADMMManyState.set_compaction`` / ``live_state``) on the GPU.

With compaction on, every launch of an armed state runs over a device-built list of the LPs of its form that are not stopped.
An LP's iterations read and write its own data only, so which workgroup runs them changes no bit: every comparison here is exact
(``np.array_equal``, ``==``) -- the compacted state against an uncompacted one driven through the same calls, the device's lists
against ``flatnonzero`` of the flags read back, the stopping iterations, residuals and steps against the CPU restatement
(tests/admm_stop_cpu.py on the oracle's iterates).  The walks are shared with test_gpu_cp_many_live.py
(tests/many_form_live_cases.py).  Needs a real MI355X: run with ``-m gpu``.
"""
import pytest

import many_form_live_cases as live
from test_admm_many_stop_host import CASES, ITERATIONS
from test_gpu_admm_many import _many_state, _problem
from test_gpu_admm_many_stop import LOOSE, TOL, _assert_fixture_iterates, _expected, form_env  # noqa: F401

pytestmark = pytest.mark.gpu


class Admm:
    """TOL stops three of the six fixtures between iterations 140 and 190, at distinct iterations; the others go on."""
    cases = CASES
    tols = TOL
    names, exact = ("iterations", "stopped", "residual", "step"), (0, 1, 2, 3)
    make = staticmethod(_many_state)
    problem = staticmethod(_problem)
    assert_iterates = staticmethod(_assert_fixture_iterates)

    @classmethod
    def arm(cls, st, every, loose=False, tight=False):
        st.set_stop(*(TOL if tight else (LOOSE if loose else cls.tols)), every)

    @staticmethod
    def state(st):
        return st.stop_state()

    @staticmethod
    def iterates(st):
        return st.x(full=True), st.lam()

    @staticmethod
    def halves(st):
        return st.sweep_step, st.multiplier_step

    @classmethod
    def expected(cls, cases, every, total):
        return _expected(cases, cls.tols, every, total)


class Loose(Admm):
    """LOOSE stops all six fixtures, between iterations 27 and 130."""
    tols = LOOSE


# ------------------------------------------------------------------ 1. on against off, call by call
@pytest.mark.parametrize("kmax", [None, 1])
@pytest.mark.parametrize("form", [None, "lds", "global"])
def test_a_compacted_state_equals_the_uncompacted_one_after_every_call(form_env, form, kmax):  # noqa: F811
    form_env(form, kmax)
    live.walk_on_against_off(Admm, form, kmax, every=1)


# ------------------------------------------------------------------ 2. both forms in one list
def test_a_form_whose_lps_have_all_stopped_launches_nothing_more(form_env):  # noqa: F811
    """potts50 is of the global form by its size; the four small LPs are all stopped after 112 iterations, potts50 after 126."""
    live.walk_both_forms(Loose, ("random0", "potts50", "potts8", "potts50", "sc105", "random2"))


# ------------------------------------------------------------------ 3. the stopping iterations are the restatement's
@pytest.mark.parametrize("every", [1, 4, 10])
def test_with_compaction_on_every_lp_stops_where_the_restatement_says(form_env, every):  # noqa: F811
    want = Admm.expected(CASES, every, ITERATIONS)
    st, off, forms, _ = live.on_and_off(Admm, [_problem(c) for c in CASES])
    try:
        for s in (st, off):
            Admm.arm(s, every)
            for k in (3, 1, 7, 50, 64, 30, ITERATIONS - 155):
                s.iterate(k)
        live.assert_state(Admm, Admm.state(st), want)
        _assert_fixture_iterates(st, CASES, want[0])
        live.assert_same(live.snapshot(Admm, st), live.snapshot(Admm, off))
        assert live.check_live(Admm, st, forms)[0].sum() == (~want[1]).sum() < len(CASES)
    finally:
        st.close()
        off.close()


# ------------------------------------------------------------------ 4. the edges of the scan, with the form predicate
@pytest.mark.parametrize("count", [1, 65, 1025, 2049])
def test_the_devices_list_is_the_flags_at_the_edges_of_the_scan(form_env, count):  # noqa: F811
    live.walk_scan_edges(Loose, ("random0", "random1", "random2"), count)


# ------------------------------------------------------------------ 5. split steps
@pytest.mark.parametrize("every", [1, 4])
def test_sweep_and_multiplier_steps_on_a_compacted_state_stop_as_whole_iterations(form_env, every):  # noqa: F811
    live.walk_split_steps(Loose, every, 110)


# ------------------------------------------------------------------ 6. unarmed
def test_an_unarmed_compacted_state_launches_the_whole_list(form_env):  # noqa: F811
    live.walk_unarmed(Admm)


# ------------------------------------------------------------------ 7. re-arming
def test_a_new_tolerance_makes_every_lp_live_again(form_env):  # noqa: F811
    live.walk_rearm(Admm)


# ------------------------------------------------------------------ 8. the C ABI
def test_the_c_abi(form_env):  # noqa: F811
    st = _many_state([_problem(c) for c in CASES])
    try:
        Loose.arm(st, 1)
        st.iterate(60)
        assert Loose.state(st)[1].any()
        live.check_c_abi(Loose, st, st._l.slp_many_admm_set_compaction, st._l.slp_many_admm_live_state, "slp_many_admm")
    finally:
        st.close()
