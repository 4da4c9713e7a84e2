"""Compaction for the Chambolle-Pock list solver (csrc/slp_cp_many.hip: ``CPManyState.set_compaction`` / ``live_state``) on the
GPU.

With compaction on, every launch of an armed state runs over a device-built list of the LPs of its form that are not stopped.
An LP's iterations read and write its own data only, so which workgroup runs them changes no bit: every comparison here is exact
(``np.array_equal``, ``==``) -- the compacted state against an uncompacted one driven through the same calls, the device's lists
against ``flatnonzero`` of the flags read back, the stopping iterations against the CPU restatements (tests/cp_stop_cpu.py,
tests/cp_gap_cpu.py on the oracle's iterates: the iterations, the flags, the step and the violation, which are exact in any order;
the certificate's two sums are in the kernel's own order and are compared with the uncompacted state's).  The walks
are shared with test_gpu_admm_many_live.py (tests/many_form_live_cases.py).  Needs a real MI355X: run with ``-m gpu``.
"""
import pytest

import many_form_live_cases as live
from test_cp_many_gap_host import TOL_FEAS, TOL_GAP, fixture_certificates
from test_cp_many_stop_host import CASES, ITERATIONS
from test_gpu_cp_many import _fixture_problem, form_env  # noqa: F401
from test_gpu_cp_many_gap import _expected as _expected_gap
from test_gpu_cp_many_stop import TOL, _assert_fixture_iterates, _expected, _make

pytestmark = pytest.mark.gpu


class _Kind:
    """What both tests of the solver share."""
    cases = CASES
    make = staticmethod(_make)
    problem = staticmethod(_fixture_problem)
    assert_iterates = staticmethod(_assert_fixture_iterates)

    @staticmethod
    def iterates(st):
        return st.x(), st.y()

    @staticmethod
    def halves(st):
        return st.primal_step, st.dual_step


class Step(_Kind):
    """The step test: TOL stops five of the six fixtures (sc50a goes on); the tight tolerance is that of the re-arming test."""
    names, exact = ("iterations", "stopped", "step"), (0, 1, 2)

    @staticmethod
    def arm(st, every, loose=False, tight=False):
        st.set_stop(1e-3 if tight else TOL, every)

    @staticmethod
    def state(st):
        return st.stop_state()

    @staticmethod
    def expected(cases, every, total):
        return _expected(cases, every, total)


class Gap(_Kind):
    """The certificate: stops four of the six fixtures within 200 iterations (sc50a and sc105 go on)."""
    names, exact = ("iterations", "stopped", "primal", "lower_bound", "violation"), (0, 1, 4)

    @staticmethod
    def arm(st, every, loose=False, tight=False):
        st.set_stop_gap(*((1e-3, 1e-3) if tight else (TOL_GAP, TOL_FEAS)), every)

    @staticmethod
    def state(st):
        return st.gap_state()

    @staticmethod
    def expected(cases, every, total):
        return _expected_gap([fixture_certificates(c) for c in cases], every, total)


KINDS = pytest.mark.parametrize("kind", [Step, Gap], ids=["step", "gap"])


# ------------------------------------------------------------------ 1. on against off, call by call
@pytest.mark.parametrize("kmax", [None, 1])
@pytest.mark.parametrize("form", [None, "lds", "global"])
@KINDS
def test_a_compacted_state_equals_the_uncompacted_one_after_every_call(form_env, kind, form, kmax):  # noqa: F811
    form_env(form, kmax)
    live.walk_on_against_off(kind, form, kmax, every=1)


# ------------------------------------------------------------------ 2. both forms in one list
def test_a_form_whose_lps_have_all_stopped_launches_nothing_more(form_env):  # noqa: F811
    """potts50 is of the global form by its size; the four small LPs are all stopped after 94 iterations, potts50 after 116."""
    live.walk_both_forms(Step, ("random0", "potts50", "potts8", "potts50", "sc105", "random1"))


# ------------------------------------------------------------------ 3. the stopping iterations are the restatement's
@pytest.mark.parametrize("every", [1, 4, 10])
@KINDS
def test_with_compaction_on_every_lp_stops_where_the_restatement_says(form_env, kind, every):  # noqa: F811
    want = kind.expected(CASES, every, ITERATIONS)
    st, off, forms, _ = live.on_and_off(kind, [_fixture_problem(c) for c in CASES])
    try:
        for s in (st, off):
            kind.arm(s, every)
            for k in (3, 1, 7, 50, 64, 30, ITERATIONS - 155):
                s.iterate(k)
        live.assert_state(kind, kind.state(st), want)
        _assert_fixture_iterates(st, CASES, want[0])
        live.assert_same(live.snapshot(kind, st), live.snapshot(kind, off))
        assert live.check_live(kind, st, forms)[0].sum() == (~want[1]).sum() < len(CASES)
    finally:
        st.close()
        off.close()


# ------------------------------------------------------------------ 4. the edges of the scan, with the form predicate
@pytest.mark.parametrize("count", [1, 65, 1025, 2049])
def test_the_devices_list_is_the_flags_at_the_edges_of_the_scan(form_env, count):  # noqa: F811
    live.walk_scan_edges(Step, ("random0", "random1", "random2"), count)


def test_the_devices_list_under_the_certificate(form_env):  # noqa: F811
    live.walk_scan_edges(Gap, ("random0", "random1", "random2"), 65)


# ------------------------------------------------------------------ 5. split steps
@pytest.mark.parametrize("every", [1, 4])
@KINDS
def test_primal_and_dual_steps_on_a_compacted_state_stop_as_whole_iterations(form_env, kind, every):  # noqa: F811
    live.walk_split_steps(kind, every, 100)


# ------------------------------------------------------------------ 6. unarmed
def test_an_unarmed_compacted_state_launches_the_whole_list(form_env):  # noqa: F811
    live.walk_unarmed(Step)


# ------------------------------------------------------------------ 7. re-arming
@KINDS
def test_a_new_tolerance_makes_every_lp_live_again(form_env, kind):  # noqa: F811
    live.walk_rearm(kind)


# ------------------------------------------------------------------ 8. the C ABI
def test_the_c_abi(form_env):  # noqa: F811
    st = _make([_fixture_problem(c) for c in CASES])
    try:
        Step.arm(st, 1)
        st.iterate(60)
        assert Step.state(st)[1].any()
        live.check_c_abi(Step, st, st._l.slp_many_cp_set_compaction, st._l.slp_many_cp_live_state, "slp_many_cp")
    finally:
        st.close()
