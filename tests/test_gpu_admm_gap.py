"""The certificate of the two single ADMM solvers on the GPU (include/slp_hip_ext_admm_gap.h; ``ADMMState`` / ``ADMMCGState`` /
``ADMMCGLPState`` / ``DeviceADMM`` ``.certificate`` / ``.set_stop_gap`` / ``.gap_state``, ``lp_admm_certified``,
``SparseLP.solve_admm_certified``).

Every form has every certificate compared with the numpy restatement (tests/admm_gap_cpu.py) on the downloaded ``x`` and
``lam``, within its derived tolerances, and every bound with the HiGHS optimum.  ``ADMMState`` and ``ADMMCGState`` hold the arrays
of ``oracle.admm_setup`` themselves.  The forms with an implicit slack column (``ADMMCGLPState``, ``DeviceADMM``) hold the same
standard form with rows normalised on the device: their iterate is mapped onto it (``admm_gap_cpu.from_implicit``) and the
tolerances carry the derived term for the scalings (``admm_gap_cpu.scale_eps``)."""
import ctypes
import functools
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest
import scipy.sparse

import admm_gap_cpu
import cp_gap_cpu
from conftest import MAX_RANKS_ON_ONE_GPU, REPO, load_golden, lp_from_golden, solver_args
from pysparselp_amd import _lib

pytestmark = pytest.mark.gpu

TOL = (1e-2, 1e-2)
TOTAL = 200
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def problem_of(name):
    return solver_args(load_golden(name))


@functools.lru_cache(maxsize=None)
def setup_of(name):
    return admm_gap_cpu.setup_of(problem_of(name))


@functools.lru_cache(maxsize=None)
def restatement_of(name):
    return admm_gap_cpu.Restatement(setup_of(name))


@functools.lru_cache(maxsize=None)
def optimum_of(name):
    res = cp_gap_cpu.highs_optimum(problem_of(name))
    assert res.status == 0
    return float(res.fun)


def make(kind, name, monkeypatch=None, reuse=0):
    """``(state, closer, explicit)``: a fresh state of the form ``kind`` on the golden LP ``name``."""
    from pysparselp_amd.ADMM import ADMMState
    from pysparselp_amd.admm_cg import ADMMCGLPState, ADMMCGState, DeviceADMM
    from pysparselp_amd.device import DeviceMatrix

    p, s = problem_of(name), setup_of(name)
    if kind in ("gs_host", "gs_host_x1"):
        st = ADMMState(s["a"], s["b"], s["c"], s["lb"], s["ub"], s["x0"], None, 2, 3)
        if kind == "gs_host_x1":
            st.set_xstep(1)
        return st, st.close, True
    if kind in ("gs_lp", "gs_lp_x1"):
        st = ADMMState.from_lp(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], None, 2, 3)
        if kind == "gs_lp_x1":
            st.set_xstep(1)
        return st, st.close, True
    if kind == "cg":
        st = ADMMCGState(s["a"], s["b"], s["c"], s["lb"], s["ub"], s["x0"], 2, 3)
        st.set_reuse(reuse)
        return st, st.close, True
    if kind in ("cg_lp", "cg_lp_strips"):
        if kind == "cg_lp_strips":
            monkeypatch.setenv("SLP_STRIP_MIN_NNZ", "1")
        st = ADMMCGLPState(*p, None, 2, 3)
        st.set_reuse(reuse)
        return st, st.close, False
    assert kind == "device"
    c, a_eq, beq, a_in, bl, bu, lb, ub = p
    m_eq = 0 if a_eq is None else a_eq.shape[0]
    k = a_in if a_eq is None else scipy.sparse.vstack([a_eq, a_in]).tocsr()
    bu2 = np.asarray(bu, dtype=np.float64) if a_eq is None else np.concatenate((beq, bu))
    bl2 = None if bl is None else np.concatenate((np.full(m_eq, -np.inf), bl))
    mat = DeviceMatrix.from_csr(k)
    st = DeviceADMM(mat, bu2, c, lb, ub, reuse=reuse, m_eq=m_eq, b_lower=bl2)

    def close():
        st.close()
        mat.close()

    return st, close, False


def whole(st):
    """x, xp (where the form has one) and lam as bytes."""
    parts = [st.x(), st.lam()]
    if hasattr(st, "xp"):
        parts.append(st.xp())
    return tuple(v.tobytes() for v in parts)


def restated(name, x, lam, explicit):
    """``admm_gap_cpu.Numbers`` for the iterate of a state on the golden LP ``name`` (an implicit form's mapped first)."""
    r = restatement_of(name)
    if explicit:
        return r.at(x, lam)
    p = problem_of(name)
    x_std, dropped = admm_gap_cpu.from_implicit(x, np.asarray(p[0]).size, 0 if p[1] is None else p[1].shape[0])
    want = r.at(x_std, lam, admm_gap_cpu.scale_eps(r))
    return want._replace(violation=max(want.violation, dropped))


def assert_numbers(name, what, numbers, want):
    primal, bound, violation = numbers
    print(name, what, "primal", primal - want.primal, want.tol_primal, "bound", bound - want.bound, want.tol_bound, "violation",
          violation - want.violation, want.tol_violation, "repaired", want.repaired)
    assert abs(primal - want.primal) <= want.tol_primal
    assert np.isfinite(bound) and abs(bound - want.bound) <= want.tol_bound
    assert abs(violation - want.violation) <= want.tol_violation
    # (HIGHS_SLACK: HiGHS's own accuracy, not a derived figure -- admm_gap_cpu)
    assert bound <= optimum_of(name) + want.tol_bound + admm_gap_cpu.HIGHS_SLACK * (1.0 + abs(optimum_of(name)))


def check_numbers(name, st, numbers, explicit):
    assert_numbers(name, type(st).__name__, numbers, restated(name, st.x(), st.lam(), explicit))


def twin_run(kind, name, monkeypatch, reuse, every, total=TOTAL, tol=TOL):
    """An unarmed twin stepped ``every`` at a time: ``(records, states, stop)`` -- the certificate and the whole iterate at every
    check, and the first check at which the decision holds on the twin's numbers."""
    st, close, explicit = make(kind, name, monkeypatch, reuse)
    try:
        records, states, stop = {}, {}, None
        for t in range(every, total + 1, every):
            st.iterate(every)
            numbers = st.certificate()
            check_numbers(name, st, numbers, explicit)
            records[t], states[t] = numbers, whole(st)
            assert st.gap_state() == (t, False, np.inf, -np.inf, np.inf)   # certificate() leaves the record alone
            if stop is None and admm_gap_cpu.decision(*numbers, *tol):
                stop = t
        return records, states, stop
    finally:
        close()


FORMS = [("gs_host", "lp_potts8", 0), ("gs_host_x1", "lp_random0", 0), ("gs_lp", "lp_random1", 0), ("gs_lp_x1", "lp_potts8", 0),
         ("gs_lp", "lp_sc50a", 0), ("gs_host", "lp_sc105", 0), ("cg", "lp_random2", 0), ("cg", "lp_potts8", 2), ("cg_lp", "lp_random0", 0),
         ("cg_lp_strips", "lp_potts8", 1), ("cg_lp_strips", "lp_random1", 4)] + [("device", "lp_potts8", r) for r in range(5)]


@pytest.mark.parametrize("kind, name, reuse", FORMS)
def test_certificates_stop_and_iterates_on_every_form(monkeypatch, kind, name, reuse):
    records, states, stop = twin_run(kind, name, monkeypatch, reuse, 10)
    st, close, _ = make(kind, name, monkeypatch, reuse)
    try:
        st.set_stop_gap(*TOL, 10)
        assert st.gap_state() == (0, False, np.inf, -np.inf, np.inf)
        st.iterate(TOTAL)
        t = TOTAL if stop is None else stop
        assert st.gap_state() == (t, stop is not None) + records[t]   # the twin's numbers bit for bit
        assert whole(st) == states[t]
        st.iterate(7)           # a stopped state enqueues nothing
        if stop is not None:
            assert st.gap_state()[0] == t and whole(st) == states[t]
    finally:
        close()


@pytest.mark.parametrize("kind, name, reuse", [("gs_lp", "lp_potts8", 0), ("cg", "lp_random0", 1), ("device", "lp_random0", 3),
                                               ("device", "lp_random0", 4)])
@pytest.mark.parametrize("every", (1, 4, 10))
def test_cadence_and_cuts(monkeypatch, kind, name, reuse, every):
    """Tolerances of 0 never stop: the armed state, cut into calls and half steps, has the unarmed state's iterate bit for bit."""
    total = 60
    plain, close_plain, _ = make(kind, name, monkeypatch, reuse)
    armed, close_armed, _ = make(kind, name, monkeypatch, reuse)
    half = (lambda s: s.sweep_step()) if hasattr(armed, "sweep_step") else (lambda s: s.xstep())
    try:
        armed.set_stop_gap(0.0, 0.0, every)
        plain.iterate(total)
        for k in (1, 2, 13):
            armed.iterate(k)
        half(armed)
        armed.multiplier_step()
        armed.iterate(0)
        armed.iterate(total - 17)
        last = total - total % every
        state = armed.gap_state()
        assert state[:2] == (total, False) and np.isfinite(state[2]) and state[4] >= 0.0
        assert whole(armed) == whole(plain)
        if last == total:
            assert armed.certificate() == state[2:]
    finally:
        close_plain()
        close_armed()


def test_arming_late_rearming_and_disarming(monkeypatch):
    kind, name = "gs_lp", "lp_potts8"
    records, states, stop = twin_run(kind, name, monkeypatch, 0, 10)
    assert stop is not None and stop >= 30
    st, close, _ = make(kind, name, monkeypatch, 0)
    try:
        st.iterate(13)                       # unarmed: counted all the same
        assert st.gap_state() == (13, False, np.inf, -np.inf, np.inf)
        st.set_stop_gap(*TOL, 10)
        st.iterate(TOTAL)
        assert st.gap_state() == (stop, True) + records[stop] and whole(st) == states[stop]
        st.set_stop_gap(0.0, 0.0, 10)        # re-armed: runs again, never stops
        st.iterate(10)
        assert st.gap_state() == (stop + 10, False) + records[stop + 10] and whole(st) == states[stop + 10]
        st.set_stop_gap(None, 0.0)           # disarmed: the record stays, nothing is evaluated
        st.iterate(10)
        assert st.gap_state() == (stop + 20, False) + records[stop + 10] and whole(st) == states[stop + 20]
    finally:
        close()


def test_refusals_at_the_c_abi(monkeypatch):
    lib = _lib.lib()
    for kind, prefix in (("gs_lp", "slp_admm"), ("cg", "slp_admm_cg")):
        st, close, _ = make(kind, "lp_potts8", monkeypatch, 0)
        stop_gap, state, certificate = (getattr(lib, prefix + "_" + f) for f in ("set_stop_gap", "gap_state", "certificate"))
        try:
            assert stop_gap(st._h, 1e-2, 1e-2, 10) == 0
            for bad in ((float("nan"), 1e-2, 1), (float("inf"), 1e-2, 1), (1e-2, -1.0, 1), (1e-2, float("nan"), 1), (1e-2, 1e-2, 0)):
                assert stop_gap(st._h, *bad) != 0 and b"tol_gap and tol_feas must be finite" in lib.slp_last_error()
            out = np.zeros(3)
            (st.sweep_step if kind == "gs_lp" else st.xstep)()
            assert stop_gap(st._h, 1e-3, 1e-3, 1) != 0 and b"between the two halves" in lib.slp_last_error()
            assert certificate(st._h, _lib.ptr(out)) != 0 and b"between the two halves" in lib.slp_last_error()
            st.multiplier_step()
            assert certificate(st._h, _lib.ptr(out)) == 0 and certificate(st._h, None) != 0
            st.iterate(9)       # the refused calls left cadence 10 and 1e-2: one check, at t = 10
            t = ctypes.c_int64(0)
            assert state(st._h, ctypes.addressof(t), None, None, None, None) == 0 and t.value == 10
            assert np.isfinite(st.gap_state()[2])
            assert state(st._h, None, None, None, None, None) == 0   # any pointer may be NULL
        finally:
            close()


@functools.lru_cache(maxsize=None)
def tiled_setup(k):
    """``lp_potts50``'s standard form (9800 rows, 17200 columns) ``k`` times on a block diagonal."""
    s = admm_gap_cpu.setup_of(problem_of("lp_potts50"))
    a = scipy.sparse.csr_matrix((s["a"].data, s["a"].indices, s["a"].indptr), shape=s["a"].shape)
    big = scipy.sparse.block_diag([a] * k, format="csr")
    big.sort_indices()
    tile = lambda v: np.tile(np.asarray(v, dtype=np.float64), k)  # noqa: E731
    csr = admm_gap_cpu.oracle.Csr(big.indptr, big.indices, big.data, big.shape)
    return dict(a=csr, b=tile(s["b"]), c=tile(s["c"]), lb=tile(s["lb"]), ub=tile(s["ub"]), x0=tile(s["x0"]))


@pytest.mark.parametrize("kind, k", [("cg", 14), ("gs_tree", 4), ("gs", 14)])
def test_sum_order_at_large_sizes(kind, k):
    """A pass has at most 131 072 slices.  14 tiles: N = 240 800 and m = 137 200, so slices of the column pass AND of the row pass
    hold a second term, and neither count is a multiple of 256.  4 tiles under ``ORDER_TREE`` (several lanes per row and per
    column in ``slp_admm``'s walks): N = 68 800 > 65 281 = 255 * 256 + 1 with a part-full last workgroup."""
    from pysparselp_amd import ORDER_TREE
    from pysparselp_amd.ADMM import ADMMState
    from pysparselp_amd.admm_cg import ADMMCGState

    s = tiled_setup(k)
    m, n = s["a"].shape
    assert n % 256 != 0 and m % 256 != 0 and (n > 131072 and m > 131072 if k == 14 else n > 65281)
    r = admm_gap_cpu.Restatement(s)
    if kind == "cg":
        st = ADMMCGState(s["a"], s["b"], s["c"], s["lb"], s["ub"], s["x0"], 2, 3)
        st.set_reuse(4)
    else:
        st = ADMMState(s["a"], s["b"], s["c"], s["lb"], s["ub"], s["x0"], None, 2, 3, ORDER_TREE if kind == "gs_tree" else 0)
    try:
        st.iterate(20)
        numbers = st.certificate()
        want = r.at(st.x(), st.lam())
        print("tiled", kind, k, n, numbers[0] - want.primal, want.tol_primal, numbers[1] - want.bound, want.tol_bound,
              numbers[2] - want.violation, want.tol_violation)
        assert abs(numbers[0] - want.primal) <= want.tol_primal and abs(numbers[1] - want.bound) <= want.tol_bound
        assert abs(numbers[2] - want.violation) <= want.tol_violation and np.isfinite(numbers[1])
    finally:
        st.close()


@pytest.mark.parametrize("xstep", ("gauss_seidel", "cg"))
def test_lp_admm_certified_and_solve_admm_certified(xstep):
    from conftest import Recorder
    from pysparselp_amd.ADMM import lp_admm, lp_admm_certified
    from pysparselp_amd.SparseLP import SparseLP

    p = problem_of("lp_potts8")
    rec = Recorder()
    x, info = lp_admm_certified(*p, *TOL, 10, nb_iter=300, callback_func=rec, xstep=xstep)
    assert info["stopped"] and info["iterations"] % 10 == 0 and sorted(info) == ["iterations", "lower_bound", "primal", "stopped", "violation"]
    assert rec.it == list(range(0, info["iterations"], 10))       # the cadence of lp_admm; no report once stopped
    assert np.array_equal(x, lp_admm(*p, nb_iter=info["iterations"] - 1, xstep=xstep))
    assert info["lower_bound"] <= optimum_of("lp_potts8") + admm_gap_cpu.HIGHS_SLACK * (1.0 + abs(optimum_of("lp_potts8")))
    lp = lp_from_golden(load_golden("lp_potts8"), SparseLP)
    x2, _ = lp.solve_admm_certified(*TOL, check_every=10, xstep=xstep, nb_iter=300)
    assert lp.stop_info == dict(info, fixed_cost=0.0) and np.array_equal(x2, x)
    x3, _ = lp.solve("admm", nb_iter=info["iterations"] - 1, xstep=xstep)
    assert np.array_equal(x3, x)
    short, info2 = lp_admm_certified(*p, 0.0, 0.0, 10, nb_iter=24, xstep=xstep)   # never met: the nb_iter + 1 iterations of lp_admm
    assert (info2["iterations"], info2["stopped"]) == (25, False) and np.array_equal(short, lp_admm(*p, nb_iter=24, xstep=xstep))


# ------------------------------------------------------------------ two ranks on one GPU
def _rank(rank, world, conn, form, cut, q):
    try:
        sys.path.insert(0, REPO)
        sys.path.insert(0, os.path.join(REPO, "tests"))
        from oracle import oracle
        from pysparselp_amd import _lib
        from pysparselp_amd.admm_cg import ADMMCGState, DeviceADMM
        from pysparselp_amd.device import DeviceMatrix

        lib = _lib.lib(0)

        @_lib.HOST_ALLREDUCE_FN
        def allreduce(buf, count, op, user):
            mine = np.ctypeslib.as_array(buf, shape=(count,))
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
        owned = None
        if form == "explicit":      # the standard form's rows cut at `cut`: slack columns among the replicated N unknowns
            s = setup_of(NAME2)
            a = scipy.sparse.csr_matrix((s["a"].data, s["a"].indices, s["a"].indptr), shape=s["a"].shape)
            cuts = (0, a.shape[0]) if world == 1 else (0, cut, a.shape[0])
            r0, r1 = cuts[rank], cuts[rank + 1]
            block = a[r0:r1]
            st = ADMMCGState(oracle.Csr(block.indptr, block.indices, block.data, block.shape), np.ascontiguousarray(s["b"][r0:r1]),
                             s["c"], s["lb"], s["ub"], s["x0"], 2, 3)
            st.set_reuse(2)
        else:                       # the LP's rows cut at `cut`: every rank holds its rows and their implicit slack columns
            c, a_eq, beq, a_in, bl, bu, lb, ub = problem_of(NAME2)
            m_eq = a_eq.shape[0]
            k = scipy.sparse.vstack([a_eq, a_in]).tocsr()
            bu2 = np.concatenate((beq, bu))
            bl2 = None if bl is None else np.concatenate((np.full(m_eq, -np.inf), bl))
            cuts = (0, k.shape[0]) if world == 1 else (0, cut, k.shape[0])
            r0, r1 = cuts[rank], cuts[rank + 1]
            owned = DeviceMatrix.from_csr(k[r0:r1])
            st = DeviceADMM(owned, np.ascontiguousarray(bu2[r0:r1]), c, lb, ub, reuse=4, m_eq=max(0, min(m_eq, r1) - r0),
                            b_lower=None if bl2 is None else np.ascontiguousarray(bl2[r0:r1]))
        st.set_stop_gap(*TOL, 10)
        states, xs, lams = [], [], []
        for _ in range(30):
            st.iterate(10)
            states.append(st.gap_state())
            xs.append(st.x())
            lams.append(st.lam())
            if states[-1][1]:
                break
        st.close()
        if owned is not None:
            owned.close()
        if world > 1:
            _lib.check(lib.slp_comm_finalize())
        q.put((rank, dict(states=states, xs=xs, lams=lams)))
    except BaseException as e:  # noqa: BLE001 -- report instead of leaving the peer blocked on the pipe
        import traceback

        q.put((rank, {"error": traceback.format_exc() + repr(e)}))


NAME2 = "lp_random0"


def _run(world, form, cut):
    assert world <= MAX_RANKS_ON_ONE_GPU
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ends = ctx.Pipe(duplex=True) if world == 2 else (None, None)
    procs = [ctx.Process(target=_rank, args=(r, world, ends[r], form, cut, q)) for r in range(world)]
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


def _whole_iterate(form, x0, x1, l0, l1):
    """The iterate of the whole LP from two ranks' downloads: the replicated unknowns once, each rank's slack columns behind
    them (implicit form), the multipliers of rank 0's rows first."""
    if form == "explicit":
        return x0, np.concatenate((l0, l1))
    n = np.asarray(problem_of(NAME2)[0]).size
    return np.concatenate((x0, x1[n:])), np.concatenate((l0, l1))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("form, cut", [("explicit", 38), ("implicit", 38), ("implicit", 7)])
def test_two_ranks_on_one_gpu(form, cut):
    """``lp_random0``'s 90 rows (10 equalities first) cut unevenly, at 38 and -- inside the equality rows -- at 7: the explicit CG
    form and ``DeviceADMM``, whose ranks hold slack columns of their own.  Both ranks report the same numbers bit for bit and the
    same stop, and the numbers are the restatement's of the whole iterate within its tolerances.  One rank's run is held to the
    same restatement on its own iterate: the two runs' iterates differ by the re-associated column sums of every iteration so
    far, for which no bound short of an error analysis of the whole ADMM recursion exists, so their numbers are not compared
    with each other beyond the stop they both reach."""
    explicit = form == "explicit"
    two, one = _run(2, form, cut), _run(1, form, 0)[0]
    a, b = two[0], two[1]
    assert a["states"] == b["states"]                      # the same numbers bit for bit, the same stop
    n = np.asarray(problem_of(NAME2)[0]).size
    for k, (state, x0, x1, l0, l1) in enumerate(zip(a["states"], a["xs"], b["xs"], a["lams"], b["lams"])):
        assert x0[:n].tobytes() == x1[:n].tobytes() and state[0] == 10 * (k + 1)
        x, lam = _whole_iterate(form, x0, x1, l0, l1)
        assert_numbers(NAME2, "two ranks, %s, t = %d" % (form, state[0]), state[2:], restated(NAME2, x, lam, explicit))
    for state, x, lam in zip(one["states"], one["xs"], one["lams"]):
        assert_numbers(NAME2, "one rank, %s, t = %d" % (form, state[0]), state[2:], restated(NAME2, x, lam, explicit))
    assert one["states"][-1][1] and a["states"][-1][1]     # both runs stop within their 300 iterations
