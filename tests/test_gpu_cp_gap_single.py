"""The certificate as the stopping test of the single Chambolle-Pock solver (csrc/slp_cp.hip: ``slp_cp_set_stop_gap``,
include/slp_hip_ext_cp_gap.h; ``CPState`` / ``DeviceCP`` ``.certificate`` / ``.set_stop_gap`` / ``.gap_state``,
``chambolle_pock_ppd_certified``, ``SparseLP.solve_certified``) on the GPU, on every form a state runs on.

The reference throughout is ``cp_gap_cpu.Restatement(problem).at(x, y)`` at the device's own downloaded ``x``, ``y``:
``primal`` and ``bound`` within its ``band`` (sums of the same terms in two fixed orders), ``violation`` exact on one GPU (every
form used here has its iterates, hence its ``K x`` chains, pinned bit for bit to the oracle by the suite) and within
``4 * 2^-52 * max_r (nnz_r + 2) (sum_j |K_rj x_j| + |b_r|)`` under two ranks, the decision exactly ``cp_gap_cpu.decision`` of the
device's three numbers and, wherever the check is decidable, the restatement's.  The stopping iterations are those of the table
tests/test_cp_gap_single_host.py pins on the CPU.  Needs a real MI355X: run with ``-m gpu``.
"""
import contextlib
import ctypes
import functools
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest
import scipy.sparse

import cp_gap_cpu
from conftest import MAX_RANKS_ON_ONE_GPU, REPO, load_golden, lp_from_golden
from test_cp_gap_single_host import TABLE, certificates_of
from test_cp_gap_single_host import problem_of as golden_problem
from test_cp_many_gap_host import (RANDOM_EVERY, RANDOM_ITERATIONS, RANDOM_LEFT_OUT, random_certificates, random_left_out,
                                   random_problems)

pytestmark = pytest.mark.gpu

TOL = (1e-2, 1e-2)
STOPS = {(name, tol): (s1, s10) for name, tol, s1, s10 in TABLE}
SWITCHES = ("SLP_CP_PACKED", "SLP_CP_ELL", "SLP_STRIP_MIN_NNZ", "SLP_CP_SPLIT", "SLP_VALUE_DICT")


@functools.lru_cache(maxsize=None)
def problem_of(name):
    """A reduced golden LP; ``lp_random0_ineq``: the inequality rows of ``lp_random0`` alone (one kind of rows, long enough for
    strip copies: the single product of the primal half)."""
    if name == "lp_random0_ineq":
        c, _, _, a_ineq, bl, bu, lb, ub = golden_problem("lp_random0")
        return (c, None, None, a_ineq, bl, bu, lb, ub)
    return golden_problem(name)


@functools.lru_cache(maxsize=None)
def restatement_of(name):
    return cp_gap_cpu.Restatement(problem_of(name))


def stacked(problem):
    """``K`` (scipy CSR, storage order kept), ``b`` and ``m_eq`` of the LP the solver holds."""
    lp = cp_gap_cpu.held_lp(problem)
    indptr = np.concatenate(([0], np.cumsum(np.bincount(lp["rows"], minlength=lp["m"])))).astype(np.int64)
    k = scipy.sparse.csr_matrix((lp["vals"], lp["cols"].astype(np.int32), indptr), shape=(lp["m"], lp["c"].size))
    return k, lp["b"], lp["m_eq"]


def host_state(problem, x0=None, order=0):
    """``CPState`` as ``chambolle_pock_ppd(setup="host")`` builds it."""
    from pysparselp_amd.ChambollePockPPD import CPState, one_sided_system

    c, a_eq, beq, a_ineq, bl, bu, lb, ub = problem
    if a_eq is not None and a_eq.shape[0] == 0:
        a_eq, beq = None, None
    ineq, b_ineq = (None, None)
    if a_ineq is not None and a_ineq.shape[0] > 0:
        ineq, b_ineq = one_sided_system(a_ineq, bl, bu)
    return CPState(c, a_eq, beq, ineq, b_ineq, lb, ub, x0, 1, 1, order)


@contextlib.contextmanager
def form(kind, name, monkeypatch, env=None, policy=0):
    """A fresh unarmed state of the golden LP ``name`` on one of the forms; yields ``(state, x_of)``."""
    from pysparselp_amd.device import ChunkedDeviceMatrix, DeviceMatrix
    from pysparselp_amd.scale import DeviceCP

    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    problem = problem_of(name)
    if kind == "host":
        st = host_state(problem)
        try:
            yield st, lambda s: s.x()
        finally:
            st.close()
        return
    k, b, m_eq = stacked(problem)
    if kind == "chunked":
        a = ChunkedDeviceMatrix.from_csr(k, chunk_entries=300, cut_at=m_eq)
        assert a.chunks >= 3
    else:
        a = DeviceMatrix.from_csr(k)
        a.set_format(policy)
        if kind == "released":
            assert a.spmv_kernel(False) != 0 and a.spmv_kernel(True) != 0
            a.release_csr()
    try:
        st = DeviceCP(a, b, problem[0], problem[6], problem[7], m_eq=m_eq)
        try:
            yield st, lambda s: s.x_reduced()
        finally:
            st.close()
    finally:
        a.close()


def violation_band(r, x):
    """``4 * 2^-52 * max_r (nnz_r + 2) (sum_j |K_rj x_j| + |b_r|)``: the bound of a re-associated ``K x - b``."""
    lp = r.lp
    if r.m == 0:
        return 0.0
    mag = np.bincount(lp["rows"], weights=np.abs(lp["vals"] * x[lp["cols"]]), minlength=r.m)
    nnz = np.bincount(lp["rows"], minlength=r.m)
    with np.errstate(invalid="ignore"):
        terms = (nnz + 2) * (mag + np.where(np.isfinite(lp["b"]), np.abs(lp["b"]), 0.0))
    return 4.0 * 2.0 ** -52 * float(np.max(terms))


def assert_certificate(r, x, y, numbers, stopped, tol, exact=True, optimum=None):
    """The device's ``(primal, bound, violation)`` and its decision against the restatement at ``(x, y)``."""
    ref = r.at(x, y)
    primal, bound, violation = numbers
    print("device", numbers, stopped, "restatement", tuple(ref))
    for got, want in ((primal, ref.primal), (bound, ref.bound)):
        if np.isfinite(want):
            assert abs(got - want) <= ref.band, (got, want, ref.band)
        else:
            assert got == want or (np.isnan(got) and np.isnan(want)), (got, want)
    if exact:
        assert violation == ref.violation or (np.isnan(violation) and np.isnan(ref.violation)), (violation, ref.violation)
    else:
        assert abs(violation - ref.violation) <= violation_band(r, x), (violation, ref.violation)
    if stopped is not None:
        assert stopped == cp_gap_cpu.decision(primal, bound, violation, *tol)
        one = cp_gap_cpu.Certificate(*(np.array([v]) for v in ref))
        if cp_gap_cpu.decidable(one, 1, *tol):
            assert stopped == cp_gap_cpu.decision(ref.primal, ref.bound, ref.violation, *tol)
    if optimum is not None and np.isfinite(ref.band):
        assert bound <= optimum + ref.band, (bound, optimum)   # the bound is a bound
    return ref


# ------------------------------------------------------------------ 1. + 6. every evaluated certificate, every form
FORMS = {
    "ell_packed": ("host", "lp_potts8", {}, 0, None),
    "ell_fp64": ("host", "lp_potts8", {"SLP_CP_PACKED": "0"}, 0, None),
    "csr_short_rows": ("host", "lp_potts8", {"SLP_CP_ELL": "0"}, 0, None),
    "csr_walk_mixed": ("host", "lp_random0", {}, 0, 0),
    "csr_walk_random1": ("host", "lp_random1", {}, 0, 0),   # the table's long runs: stops at 174 and 156
    "csr_walk_random2": ("host", "lp_random2", {}, 0, 0),
    "strips_dict_split1": ("device", "lp_random0", {"SLP_STRIP_MIN_NNZ": "1"}, 0, 1),
    "strips_fp64_split1": ("device", "lp_random0", {"SLP_STRIP_MIN_NNZ": "1"}, 1, 1),
    "strips_dict_masked": ("device", "lp_random0", {"SLP_STRIP_MIN_NNZ": "1", "SLP_CP_SPLIT": "masked"}, 0, 2),
    "strips_fp64_masked": ("device", "lp_random0", {"SLP_STRIP_MIN_NNZ": "1", "SLP_CP_SPLIT": "masked"}, 1, 2),
    "device_potts": ("device", "lp_potts8", {}, 0, 0),
    "released": ("released", "lp_random0", {"SLP_STRIP_MIN_NNZ": "1"}, 0, 2),
    "chunked_cut": ("chunked", "lp_random0", {"SLP_STRIP_MIN_NNZ": "1"}, 0, 1),
}


@pytest.mark.parametrize("case", list(FORMS))
def test_every_evaluated_certificate_on_every_form(monkeypatch, case):
    kind, name, env, policy, split = FORMS[case]
    stop = STOPS[(name, TOL)][0]
    r, problem = restatement_of(name), problem_of(name)
    optimum = cp_gap_cpu.highs_optimum(problem).fun
    with form(kind, name, monkeypatch, env, policy) as (st, x_of):
        if split is not None and kind != "host":
            assert st.split_form() == split
        assert st.gap_state() == (0, False, np.inf, -np.inf, np.inf)
        st.set_stop_gap(*TOL, 1)
        for t in range(1, stop + 6):
            st.iterate(1)
            iterations, stopped, *numbers = st.gap_state()
            assert iterations == min(t, stop) and stopped == (t >= stop), (t, iterations, stopped)
            if t <= stop:
                x, y = x_of(st), st.y()
                assert_certificate(r, x, y, numbers, stopped, TOL, optimum=optimum)
        exact = cp_gap_cpu.exact_bound(problem, y)
        assert abs(exact - numbers[1]) <= r.at(x, y).band, (exact, numbers[1])
        assert st.certificate() == tuple(numbers)   # the same launches on the same iterate


@pytest.mark.parametrize("kind, name, env", [("host", "lp_sc50a", {}), ("device", "lp_random0_ineq", {"SLP_STRIP_MIN_NNZ": "1"}),
                                             ("released", "lp_random0_ineq", {"SLP_STRIP_MIN_NNZ": "1"})])
def test_numbers_only(monkeypatch, kind, name, env):
    """``lp_sc50a`` does not stop within 400 iterations (the table); the inequality rows of ``lp_random0`` alone run the primal
    half as ONE product over the strip copy of ``K^T`` (split form 0).  Tolerances of 0: 50 iterations, numbers only."""
    r, problem = restatement_of(name), problem_of(name)
    optimum = cp_gap_cpu.highs_optimum(problem).fun
    with form(kind, name, monkeypatch, env) as (st, x_of):
        if kind != "host":
            assert st.split_form() == 0 and st.a.spmv_kernel(True) != 0
        st.set_stop_gap(0.0, 0.0, 1)
        for t in range(1, 51):
            st.iterate(1)
            iterations, stopped, *numbers = st.gap_state()
            assert (iterations, stopped) == (t, False)
            assert_certificate(r, x_of(st), st.y(), numbers, stopped, (0.0, 0.0), optimum=optimum)


# ------------------------------------------------------------------ 2. edge shapes
def test_edge_shapes_of_the_seeded_list():
    from pysparselp_amd import ORDER_SEQUENTIAL

    left_out = random_left_out()
    assert len(left_out) <= RANDOM_LEFT_OUT
    for k, (problem, cert) in enumerate(zip(random_problems(), random_certificates())):
        r = cp_gap_cpu.Restatement(problem)
        st = host_state(problem, order=ORDER_SEQUENTIAL)   # rows of up to 40 entries: the oracle's chains, as the list solver's
        try:
            st.set_stop_gap(*TOL, RANDOM_EVERY)
            st.iterate(RANDOM_ITERATIONS)
            iterations, stopped, *numbers = st.gap_state()
            assert_certificate(r, st.x(), st.y(), numbers, stopped, TOL)   # the record is that of the iterate it stands at
            if k not in left_out:
                want = cp_gap_cpu.gap_state(cert, *TOL, RANDOM_EVERY, RANDOM_ITERATIONS)
                assert (iterations, stopped) == (want[0], want[1]), (k, iterations, stopped, want)
        finally:
            st.close()


# ------------------------------------------------------------------ 3. cadence and cuts
def _bits(st, x_of):
    return x_of(st).tobytes(), st.y().tobytes()


@pytest.mark.parametrize("tol", (TOL, (0.0, 0.0)), ids=("stops", "never"))
@pytest.mark.parametrize("every", (1, 4, 10))
def test_cadence_and_cuts(monkeypatch, every, tol):
    """``lp_random1`` stops at 174 (cadence 1) to 180 (cadence 10) of 200 iterations at ``1e-2 / 1e-2`` and never at tolerances of
    0: one call of 200, calls of 7 (28 of them and one of 4) and 200 pairs of half steps give the same records and iterates."""
    name, total = "lp_random1", 200
    _, _, cert = certificates_of(name)
    want = cp_gap_cpu.gap_state(cert, *tol, every, total)
    assert want[:2] == ((STOPS[(name, TOL)][0] if every == 1 else want[0], True) if tol == TOL else (total, False))
    assert want[0] >= 174
    with form("host", name, monkeypatch) as (one, x_of), form("host", name, monkeypatch) as (cut, _), \
            form("host", name, monkeypatch) as (halves, _):
        for st in (one, cut, halves):
            st.set_stop_gap(*tol, every)
        one.iterate(total)
        for k in [7] * (total // 7) + [total % 7]:
            cut.iterate(k)
        for _ in range(total):
            halves.primal_step()
            halves.dual_step()
        got = one.gap_state()
        assert got[:2] == want[:2], (got, want)
        assert cut.gap_state() == got and halves.gap_state() == got
        assert _bits(cut, x_of) == _bits(one, x_of) == _bits(halves, x_of)
        if got[1]:   # a stopped state does not move
            before = _bits(one, x_of)
            one.iterate(20)
            one.primal_step()
            one.dual_step()
            assert one.gap_state() == got and _bits(one, x_of) == before


def test_arming_late_rearming_and_disarming(monkeypatch):
    name = "lp_potts8"
    _, _, cert = certificates_of(name)
    with form("host", name, monkeypatch) as (st, x_of), form("host", name, monkeypatch) as (plain, _):
        st.iterate(25)
        assert st.gap_state() == (25, False, np.inf, -np.inf, np.inf)   # t counts from the state's birth, armed or not
        st.set_stop_gap(*TOL, 10)
        st.iterate(200)
        want = cp_gap_cpu.gap_state(cert, *TOL, 10, 225, after=25)
        assert st.gap_state()[:2] == want[:2] == (60, True)
        plain.iterate(60)
        assert _bits(st, x_of) == _bits(plain, x_of)
        st.set_stop_gap(1e-3, 1e-3, 1)    # a tighter tolerance lets it go on
        assert st.gap_state()[:2] == (60, False)
        st.iterate(200)
        assert st.gap_state()[:2] == (STOPS[(name, (1e-3, 1e-3))][0], True)
        record = st.gap_state()[2:]
        st.set_stop_gap(None, None)       # so does disarming; the record stays
        st.iterate(5)
        assert st.gap_state() == (101, False) + record
        plain.iterate(41)
        assert _bits(st, x_of) == _bits(plain, x_of)


# ------------------------------------------------------------------ 4. armed changes nothing else
@pytest.mark.parametrize("kind, env", [("host", {}), ("device", {"SLP_STRIP_MIN_NNZ": "1"})])
def test_an_armed_state_has_the_iterates_of_an_unarmed_one(monkeypatch, kind, env):
    name = "lp_random1"
    with form(kind, name, monkeypatch, env) as (armed, x_of), form(kind, name, monkeypatch, env) as (plain, _):
        armed.set_stop_gap(0.0, 0.0, 1)
        armed.iterate(120)   # the ELL / CSR path replays its captured graph for an unarmed state, an armed one is cut at every check
        armed.set_stop_gap(0.0, 0.0, 10)
        armed.iterate(80)
        plain.iterate(200)
        assert armed.gap_state()[:2] == (200, False) and plain.gap_state() == (200, False, np.inf, -np.inf, np.inf)
        assert _bits(armed, x_of) == _bits(plain, x_of)


# ------------------------------------------------------------------ 5. certificate() leaves the state alone
@pytest.mark.parametrize("kind, env", [("host", {}), ("device", {"SLP_STRIP_MIN_NNZ": "1"})])
def test_certificate_leaves_the_state_alone(monkeypatch, kind, env):
    name = "lp_random0"
    r = restatement_of(name)
    with form(kind, name, monkeypatch, env) as (st, x_of), form(kind, name, monkeypatch, env) as (twin, _):
        for s in (st, twin):
            s.set_stop_gap(*TOL, 10)
            s.iterate(27)
        before, state = _bits(st, x_of), st.gap_state()
        numbers = st.certificate()
        assert_certificate(r, x_of(st), st.y(), numbers, None, TOL)   # of iteration 27, which no check evaluates
        assert numbers != state[2:]
        assert _bits(st, x_of) == before and st.gap_state() == state
        st.primal_step()            # also between the halves of a reporting iteration: the report's numbers stay
        report = st.report()
        st.certificate()
        assert np.array_equal(st.report(), report, equal_nan=True)
        st.dual_step()
        twin.iterate(1)
        for s in (st, twin):
            s.iterate(9)
        assert _bits(st, x_of) == _bits(twin, x_of) and st.gap_state() == twin.gap_state()


# ------------------------------------------------------------------ 7. drivers
@pytest.mark.parametrize("setup", ("host", "device"))
def test_chambolle_pock_ppd_certified(setup):
    from pysparselp_amd.ChambollePockPPD import chambolle_pock_ppd, chambolle_pock_ppd_certified

    problem = problem_of("lp_potts8")
    reports = []
    x, _, info = chambolle_pock_ppd_certified(*problem, *TOL, check_every=10, setup=setup, nb_max_iter=400,
                                              callback_func=lambda niter, *rest: reports.append(niter))
    assert info["iterations"] == 60 and info["stopped"] is True and reports == list(range(0, 60, 10))
    ref, _ = chambolle_pock_ppd(*problem, nb_max_iter=60, setup=setup)
    assert x.tobytes() == ref.tobytes()
    assert cp_gap_cpu.decision(info["primal"], info["lower_bound"], info["violation"], *TOL)
    x, _, info = chambolle_pock_ppd_certified(*problem, *TOL, setup=setup, max_time=0.0)
    assert info == dict(iterations=0, stopped=False, primal=np.inf, lower_bound=-np.inf, violation=np.inf)


@pytest.mark.parametrize("setup", ("host", "device"))
def test_solve_certified(setup):
    from pysparselp_amd.SparseLP import SparseLP

    d = load_golden("lp_potts8")
    lp = lp_from_golden(d, SparseLP)
    # some variables fixed where a solution has them (the oracle's iterate after 2000 iterations), so that the LP stays feasible
    xs, _ = cp_gap_cpu.iterates(problem_of("lp_potts8"), 2000)
    assert xs[-1].size == lp.nb_variables
    fixed = np.arange(0, lp.nb_variables, 9)
    lp.upper_bounds[fixed] = lp.lower_bounds[fixed] = xs[-1][fixed]
    x = lp.solve_certified(*TOL, check_every=10, get_timing=False, nb_iter=2000, setup=setup)
    info = lp.stop_info
    print(info)
    assert info["stopped"] and info["iterations"] % 10 == 0 and 0 < info["iterations"] < 2000
    assert info["fixed_cost"] == float(np.dot(lp.costsvector[fixed], lp.lower_bounds[fixed]))
    assert lp.itrn_curve == list(range(0, info["iterations"], 10))   # the curves end at the stop
    assert cp_gap_cpu.decision(info["primal"], info["lower_bound"], info["violation"], *TOL)
    other = lp_from_golden(d, SparseLP)
    other.upper_bounds[fixed] = other.lower_bounds[fixed] = xs[-1][fixed]
    ref = other.solve("chambolle_pock_ppd", get_timing=False, nb_iter=info["iterations"], setup=setup)
    assert x.tobytes() == ref.tobytes()


# ------------------------------------------------------------------ 9. refusals at the C ABI
def test_refusals_at_the_c_abi(monkeypatch):
    from pysparselp_amd import _lib

    with form("host", "lp_potts8", monkeypatch) as (st, x_of):
        lib = st._l
        out = np.zeros(3)
        assert lib.slp_cp_certificate(None, _lib.ptr(out)) != 0 and lib.slp_cp_certificate(st._h, None) != 0
        assert lib.slp_cp_set_stop_gap(None, 1e-2, 1e-2, 1) != 0
        assert lib.slp_cp_gap_state(None, None, None, None, None, None) != 0
        st.set_stop_gap(*TOL, 10)
        st.iterate(30)
        state = st.gap_state()
        for bad in ((np.nan, 1e-2, 1), (np.inf, 1e-2, 1), (1e-2, np.nan, 1), (1e-2, np.inf, 1), (1e-2, -1e-2, 1), (1e-2, 1e-2, 0),
                    (1e-2, 1e-2, -4)):
            assert lib.slp_cp_set_stop_gap(st._h, *bad) != 0, bad
            assert b"slp_cp_set_stop_gap" in lib.slp_last_error()
        assert st.gap_state() == state
        st.iterate(200)     # ... and keeps what it had: cadence 10, 1e-2
        assert st.gap_state()[:2] == (60, True)
        assert lib.slp_cp_gap_state(st._h, None, None, None, None, None) == 0   # any pointer may be NULL
        t = ctypes.c_int64(0)
        assert lib.slp_cp_gap_state(st._h, ctypes.addressof(t), None, None, None, None) == 0 and t.value == 60


# ------------------------------------------------------------------ 8. two ranks on one GPU
def _rank(rank, world, conn, cuts, q):
    try:
        sys.path.insert(0, REPO)
        sys.path.insert(0, os.path.join(REPO, "tests"))
        from pysparselp_amd import _lib
        from pysparselp_amd.device import DeviceMatrix
        from pysparselp_amd.scale import DeviceCP

        lib = _lib.lib(0)
        sizes = []

        @_lib.HOST_ALLREDUCE_FN
        def allreduce(buf, count, op, user):
            mine = np.ctypeslib.as_array(buf, shape=(count,))
            sizes.append(int(count))
            if rank == 0:  # one side sends first, the other receives first: no deadlock
                conn.send_bytes(mine.tobytes())
                other = np.frombuffer(conn.recv_bytes(), dtype=np.float64)
                res = np.maximum(mine, other) if op == 1 else mine + other
            else:
                other = np.frombuffer(conn.recv_bytes(), dtype=np.float64)
                conn.send_bytes(mine.tobytes())
                res = np.maximum(other, mine) if op == 1 else other + mine  # rank 0's term first on both sides
            assert other.size == count, (other.size, count)
            mine[:] = res
            return 0

        if world > 1:
            _lib.check(lib.slp_comm_init_host(world, rank, allreduce, None))
        problem = problem_of("lp_random0")
        k, b, m_eq = stacked(problem)
        r0, r1 = cuts[rank], cuts[rank + 1]
        a = DeviceMatrix.from_csr(k[r0:r1])
        st = DeviceCP(a, b[r0:r1], problem[0], problem[6], problem[7], m_eq=max(0, min(m_eq, r1) - r0))
        st.set_stop_gap(*TOL, 10)
        states, xs, ys, counts = [], [], [], []
        for _ in range(40):
            mark = len(sizes)
            st.iterate(10)
            counts.append(sizes[mark:])
            states.append(st.gap_state())
            xs.append(st.x_reduced())
            ys.append(st.y())
            if states[-1][1]:
                break
        st.close()
        a.close()
        if world > 1:
            _lib.check(lib.slp_comm_finalize())
        q.put((rank, dict(states=states, xs=xs, ys=ys, counts=counts)))
    except BaseException as e:  # noqa: BLE001 -- report instead of leaving the peer blocked on the pipe
        import traceback

        q.put((rank, {"error": traceback.format_exc() + repr(e)}))


def _run(world, cuts):
    assert world <= MAX_RANKS_ON_ONE_GPU
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ends = ctx.Pipe(duplex=True) if world == 2 else (None, None)
    procs = [ctx.Process(target=_rank, args=(r, world, ends[r], cuts, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    res = {}
    for _ in range(world):
        rank, out = q.get(timeout=300)
        assert "error" not in out, out["error"]
        res[rank] = out
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    return res


@pytest.mark.timeout(600)
@pytest.mark.parametrize("cut", (38, 90))
def test_two_ranks_on_one_gpu(cut):
    """``lp_random0``'s 90 rows as 38 + 52 (the 10 equality rows on rank 0) and as 90 + 0 (an empty block)."""
    name = "lp_random0"
    r, n = restatement_of(name), problem_of(name)[0].size
    _, _, cert = certificates_of(name)
    two = _run(2, (0, cut, 90))
    a, b = two[0], two[1]
    assert a["states"] == b["states"]                      # the same numbers bit for bit, the same stop
    assert a["states"][-1][1] and len(a["states"]) < 40
    for k, (state, x, y0, y1) in enumerate(zip(a["states"], a["xs"], a["ys"], b["ys"])):
        assert x.tobytes() == b["xs"][k].tobytes()
        assert state[0] == 10 * (k + 1)
        assert_certificate(r, x, np.concatenate((y0, y1)), state[2:], state[1], TOL, exact=False)
    # what a check adds to the ten all-reduces of n doubles of its iterations: one of n doubles and the two scalar reductions
    assert a["counts"] == b["counts"] and all(c == [n] * 11 + [1, 1] for c in a["counts"]), a["counts"][0]
    stop = a["states"][-1][0]
    single = cp_gap_cpu.stopping_iteration(cert, *TOL, 10)
    if all(cp_gap_cpu.decidable(cert, t, *TOL) for t in cp_gap_cpu.checks(max(stop, single), 10)):
        assert stop == single
