"""Dual gradient ascent on the GPU (csrc/slp_dga.hip) against the reference's results (tests/golden/dga.npz, each case up to
its agreement horizon), its captured line-search calls, an integer-valued LP whose sums do not depend on their order over
every product format, the reference's recorded curves through SparseLP.solve, and the edge cases of its calling contract.
Every case runs with the fused one-workgroup search and with the general (radix sort, tiled scans) search forced."""
import json
import os

import numpy as np
import pytest
import scipy.sparse

from conftest import GOLDEN, Recorder, csr_of, load_golden, lp_from_golden
from dga_cpu import dga_cpu, dual_energy
from test_dga_host import CASES, dga_args

pytestmark = pytest.mark.gpu

PATHS = ("fused", "general")


class LP:
    """The attributes dual_gradient_ascent reads."""

    def __init__(self, c, a_eq, b_eq, a_ineq, b_upper, lb, ub, b_lower=None):
        self.costsvector, self.a_equalities, self.b_equalities = c, a_eq, b_eq
        self.a_inequalities, self.b_upper, self.b_lower = a_ineq, b_upper, b_lower
        self.lower_bounds, self.upper_bounds = lb, ub


def start_of(a_eq, a_ineq):
    """The reference's start (seed 0) and the generator its tie draws continue."""
    rs = np.random.RandomState(0)
    y_eq = -rs.rand(a_eq.shape[0])
    y_ineq = np.abs(rs.rand(a_ineq.shape[0])) if a_ineq is not None else np.zeros(0)
    return y_eq, y_ineq, rs


def device_state(args, path, mat=None):
    from pysparselp_amd.DualGradientAscent import DeviceDGA
    from pysparselp_amd.device import DeviceMatrix

    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = args
    y_eq, y_ineq, rs = start_of(a_eq, a_ineq)
    own = mat is None
    if own:
        mat = DeviceMatrix.from_blocks(a_eq, a_ineq, c.size)
    b = np.concatenate((b_eq, b_upper if a_ineq is not None else np.zeros(0)))
    state = DeviceDGA(mat, b, c, lb, ub, np.concatenate((y_eq, y_ineq)), m_eq=a_eq.shape[0], draws=rs.random_sample, path=path)
    assert state.path() == path
    return state, (mat if own else None)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", CASES)
def test_gpu_dga_matches_the_reference_up_to_the_horizon(case, path):
    g = load_golden("dga")
    horizon = int(g[f"{case}_horizon"])
    keep = [int(i) for i in g[f"{case}_it"]]
    state, mat = device_state(dga_args(load_golden("lp_" + case)), path)
    try:
        done = 0
        for k, it in enumerate(keep):
            if it > horizon:
                break
            state.iterate(it + 1 - done)
            done = it + 1
            flags, draws, _, iters = state.status()
            y_eq, y_ineq = state.y()
            assert flags == 0 and iters == done
            assert np.array_equal(state.x(), g[f"{case}_x"][k]), it
            assert np.array_equal(y_eq, g[f"{case}_yeq"][k]), it
            assert np.array_equal(y_ineq, g[f"{case}_yineq"][k]), it
            assert draws == int(g[f"{case}_draws"][k]), it
        assert done == horizon + 1
    finally:
        state.close()
        mat.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", CASES)
def test_gpu_line_search_reproduces_the_captured_calls(case, path):
    from pysparselp_amd.DualGradientAscent import exact_dual_line_search

    g = load_golden("dga")
    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = dga_args(load_golden("lp_" + case))
    seen = {0: 0, 1: 0}
    assert g[f"{case}_ls_it"].size > 0
    for k, kind in enumerate(g[f"{case}_ls_kind"]):
        kind = int(kind)
        direction = g[f"{case}_ls_g_ineq" if kind == 0 else f"{case}_ls_g_eq"][seen[kind]]
        seen[kind] += 1
        draw = g[f"{case}_ls_draw"][k]
        a, b = (a_ineq, b_upper) if kind == 0 else (a_eq, b_eq)
        step = exact_dual_line_search(scipy.sparse.csr_matrix(direction), a, b, g[f"{case}_ls_cbar"][k], ub, lb,
                                      draws=[] if np.isnan(draw) else [draw], path=path)
        assert step == g[f"{case}_ls_step"][k], (k, step, g[f"{case}_ls_step"][k])


# ---- integer-valued LPs: every term of the derivative is an exactly representable integer (or half-integer), so the search does
# not depend on the order of its sums at any size.  The shapes are those of tests/test_gpu_format_matrix.py: TALL (n = 2e5: ~200
# scan tiles and a many-workgroup sort on the general path; ~1 entry per row and 4096-column cell in both orientations) and
# STRIPS (30 entries per row over 8 LDS strips); a tenth of the rows are equalities.
INT_LPS = {"tall": dict(m=40_000, n=200_000, per_row=50, m_eq=4_000, seed=11),
           "strips": dict(m=14_000, n=30_000, per_row=30, m_eq=1_400, seed=12)}
INT_ITERS = 50
# (shape, switches, kernel code in both orientations, row chunks: None / "cut" at m_eq / "chunked" elsewhere): the formats that
# file enumerates for these shapes, with its chunked variants
FORMATS = {
    "csr": ("tall", {}, 0, None),
    "tall_dict": ("tall", {"SLP_STRIP_MIN_NNZ": "1", "SLP_VALUE_DICT": "1"}, 6, None),
    "tall_fp64": ("tall", {"SLP_STRIP_MIN_NNZ": "1", "SLP_VALUE_DICT": "0"}, 7, None),
    "tall_dict_cut": ("tall", {"SLP_STRIP_MIN_NNZ": "1", "SLP_VALUE_DICT": "1"}, 6, "cut"),
    "fp64": ("strips", {"SLP_STRIP_MIN_NNZ": "1", "SLP_VALUE_DICT": "0"}, 1, None),
    "pairs": ("strips", {"SLP_STRIP_MIN_NNZ": "1", "SLP_VALUE_DICT": "1", "SLP_DICT_VARIANT": "1"}, 2, None),
    "quads": ("strips", {"SLP_STRIP_MIN_NNZ": "1", "SLP_VALUE_DICT": "1", "SLP_DICT_VARIANT": "2"}, 3, None),
    "pairs_chunked": ("strips", {"SLP_STRIP_MIN_NNZ": "1", "SLP_VALUE_DICT": "1", "SLP_DICT_VARIANT": "1"}, 2, "chunked"),
}
ALL_SWITCHES = ("SLP_STRIP_MIN_NNZ", "SLP_VALUE_DICT", "SLP_DICT_VARIANT", "SLP_TALL", "SLP_TALL_R", "SLP_STRIP_SPLIT", "SLP_TALL_SPLIT")
_INT = {}


def integer_lp(shape):
    if shape not in _INT:
        p = INT_LPS[shape]
        rng = np.random.RandomState(p["seed"])
        m, n, k = p["m"], p["n"], p["per_row"]
        cols = (np.arange(k) * (n // k) + rng.randint(0, n // k, size=(m, k))).astype(np.int32)   # one per stratum: sorted, distinct
        vals = np.round(100 * rng.randn(m, k))
        vals[vals == 0] = 1.0
        a = scipy.sparse.csr_matrix((vals.ravel(), cols.ravel(), np.arange(0, m * k + 1, k)), shape=(m, n))
        lb = rng.randint(-5, 1, size=n).astype(np.float64)
        ub = lb + rng.randint(1, 10, size=n)
        xf = lb + np.floor(rng.rand(n) * (ub - lb + 1))
        ax = a @ xf
        b = ax + rng.randint(0, 50, size=m)
        b[:p["m_eq"]] = ax[:p["m_eq"]]
        c = np.round(100 * rng.randn(n))
        a_eq, a_ineq = a[:p["m_eq"]].tocsr(), a[p["m_eq"]:].tocsr()
        args = (c, a_eq, b[:p["m_eq"]], a_ineq, b[p["m_eq"]:], lb, ub)
        ref = dga_cpu(*args, nb_max_iter=INT_ITERS, order="reference", keep=[0, 9, INT_ITERS - 1])
        _INT[shape] = (args, ref, a)
    return _INT[shape]


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_gpu_dga_integer_lp_on_every_product_format(monkeypatch, fmt):
    from pysparselp_amd.device import ChunkedDeviceMatrix, DeviceMatrix

    shape, switches, code, chunks = FORMATS[fmt]
    args, ref, stacked = integer_lp(shape)
    for name in ALL_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in switches.items():
        monkeypatch.setenv(name, value)
    if chunks:   # row chunks whose CSR is released: the products run over composites of the chunks' copies
        mat = ChunkedDeviceMatrix.from_csr(stacked, chunk_entries=stacked.nnz // 2 + 1,
                                           cut_at=INT_LPS[shape]["m_eq"] if chunks == "cut" else 0)
        assert mat.chunks == (3 if chunks == "cut" else 2)
    else:
        mat = DeviceMatrix.from_blocks(args[1], args[3], args[0].size)
    state, _ = device_state(args, "general", mat=mat)
    try:
        assert (mat.spmv_kernel(False), mat.spmv_kernel(True)) == (code, code)
        done = 0
        for it in sorted(ref):
            if it < 0:
                continue
            state.iterate(it + 1 - done)
            done = it + 1
            x, y_eq, y_ineq, draws = ref[it]
            flags, got_draws, _, _ = state.status()
            ge, gi = state.y()
            assert flags == 0 and got_draws == draws, it
            assert np.array_equal(state.x(), x) and np.array_equal(ge, y_eq) and np.array_equal(gi, y_ineq), it
    finally:
        state.close()
        mat.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case,key", [("sc105", "netlib_curves_SC105.json"), ("potts50", "test_pott_segmentation_curves.json")])
def test_gpu_dga_reference_golden_curves(monkeypatch, case, key, path):
    """tests/test_netlib.py:119-125 of the reference (common prefix, 7 decimals), method dual_gradient_ascent, through
    SparseLP.solve; the prefix ends with the case's horizon."""
    from pysparselp_amd.SparseLP import SparseLP

    monkeypatch.setenv("SLP_DGA_PATH", path)
    horizon = int(load_golden("dga")[f"{case}_horizon"])
    d = load_golden("lp_" + case)
    lp = lp_from_golden(d, SparseLP)
    lp.solve(method="dual_gradient_ascent", get_timing=True, nb_iter=horizon + 1, max_time=None, ground_truth=d["gt"],
             ground_truth_indices=d["gt_idx"], plot_solution=None, nb_iter_plot=500)
    ref = json.load(open(os.path.join(GOLDEN, "ref_dga_curves.json")))[key]
    got = lp.distance_to_ground_truth
    points = min(len(got), len(ref))
    assert lp.itrn_curve == list(range(0, horizon + 1, 100))
    assert points >= (2 if case == "sc105" else horizon // 100 + 1)
    assert len(lp.pobj_curve) == len(lp.max_violated_constraint) == len(lp.opttime_curve) == len(got)
    np.testing.assert_almost_equal(got[:points], ref[:points])


# ---- edge cases ---------------------------------------------------------------------------------------------------------------

def _reference_triple(lp, nb_max_iter, y_eq=None, y_ineq=None):
    out = dga_cpu(lp.costsvector, lp.a_equalities, lp.b_equalities, lp.a_inequalities, lp.b_upper, lp.lower_bounds, lp.upper_bounds,
                  nb_max_iter=nb_max_iter, order="reference", y_eq=y_eq, y_ineq=y_ineq)
    return out[max(out)]


def _assert_triple(got, ref):
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert (got[2] is None and ref[2] is None) or np.array_equal(got[2], ref[2])


@pytest.mark.parametrize("path", PATHS)
def test_gpu_dga_one_kind_of_rows_and_given_multipliers(monkeypatch, path):
    from pysparselp_amd.DualGradientAscent import dual_gradient_ascent

    monkeypatch.setenv("SLP_DGA_PATH", path)
    # no equality rows (Potts-8 has none: a 0-row block, as the reference needs it); 0-row inequality block dropped = None
    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = dga_args(load_golden("lp_potts8"))
    assert a_eq.shape[0] == 0
    lp = LP(c, a_eq, b_eq, a_ineq, b_upper, lb, ub)
    _assert_triple(dual_gradient_ascent(None, lp, nb_max_iter=30), _reference_triple(lp, 30))
    # no inequality rows: the equality rows of SC50A alone
    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = dga_args(load_golden("lp_sc50a"))
    lp = LP(c, a_eq, b_eq, None, None, lb, ub)
    got = dual_gradient_ascent(None, lp, nb_max_iter=30)
    assert got[2] is None
    _assert_triple(got, _reference_triple(lp, 30))
    # the caller's multipliers
    lp = LP(c, a_eq, b_eq, a_ineq, b_upper, lb, ub)
    rs = np.random.RandomState(3)
    y_eq, y_ineq = rs.randn(a_eq.shape[0]), rs.rand(a_ineq.shape[0])
    keep_eq, keep_ineq = y_eq.copy(), y_ineq.copy()
    _assert_triple(dual_gradient_ascent(None, lp, nb_max_iter=30, y_eq=y_eq, y_ineq=y_ineq), _reference_triple(lp, 30, y_eq, y_ineq))
    assert np.array_equal(y_eq, keep_eq) and np.array_equal(y_ineq, keep_ineq)


def test_gpu_dga_dual_infeasible_start_returns_at_once():
    """A variable without an upper bound whose reduced cost is negative at the start: energy -inf (:133-139)."""
    from pysparselp_amd.DualGradientAscent import dual_gradient_ascent

    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = dga_args(load_golden("lp_sc50a"))
    y_eq, y_ineq, _ = start_of(a_eq, a_ineq)
    c_bar = (c + y_eq * a_eq) + y_ineq * a_ineq
    j = int(np.flatnonzero(c_bar < 0)[0])
    ub = ub.copy()
    ub[j] = np.inf
    assert dual_energy(c, a_eq, b_eq, a_ineq, b_upper, lb, ub, y_eq, y_ineq) == -np.inf
    lp = LP(c, a_eq, b_eq, a_ineq, b_upper, lb, ub)
    rec = Recorder()
    x, ye, yi = dual_gradient_ascent(None, lp, nb_max_iter=50, callback_func=rec)
    ref = dga_cpu(c, a_eq, b_eq, a_ineq, b_upper, lb, ub, nb_max_iter=50)
    assert sorted(ref) == [-1] and rec.it == []
    assert np.array_equal(x, ref[-1][0]) and x[j] == np.inf
    assert np.array_equal(ye, y_eq) and np.array_equal(yi, y_ineq)


def test_gpu_dga_callbacks_and_max_time():
    from pysparselp_amd.DualGradientAscent import dual_gradient_ascent

    lp = LP(*dga_args(load_golden("lp_sc50a")))
    rec = Recorder()
    out = dual_gradient_ascent(None, lp, nb_max_iter=250, callback_func=rec, nb_iter_plot=7)
    assert rec.it == [0, 100, 200] and rec.e1 == [0, 0, 0] and rec.veq == [0, 0, 0]
    _assert_triple(out, _reference_triple(lp, 250))
    for it, x in zip(rec.it, rec.x):   # the x of the top of that iteration
        assert np.array_equal(x, _reference_triple(lp, it + 1)[0])
    rec = Recorder()
    out = dual_gradient_ascent(None, lp, nb_max_iter=250, callback_func=rec, max_time=1e-9)   # ends at the first callback boundary
    assert rec.it == [0]
    _assert_triple(out, _reference_triple(lp, 1))


@pytest.mark.parametrize("path", PATHS)
def test_gpu_dga_refills_of_the_draw_buffer_do_not_change_the_result(path):
    args = dga_args(load_golden("lp_sc50a"))
    runs = []
    for chunks in ([120], [1] * 30 + [7] * 10 + [20]):
        state, mat = device_state(args, path)
        try:
            for k in chunks:
                state.iterate(k)
            flags, draws, _, iters = state.status()
            assert flags == 0 and iters == 120 and draws > 0
            runs.append((state.x(), *state.y(), draws))
        finally:
            state.close()
            mat.close()
    for p, q in zip(runs[0], runs[1]):
        assert np.array_equal(p, q)
    # a buffer that could run dry stops the call early, sticky bit 4 until the next push
    state, mat = device_state(args, path)
    try:
        state.push_random(np.random.RandomState(5).random_sample(6))
        state.iterate(10, refill=False)
        flags, _, _, iters = state.status()
        assert flags & 4 and iters == 3
    finally:
        state.close()
        mat.close()


@pytest.mark.parametrize("path", PATHS)
def test_gpu_dga_empty_breakpoint_set_sets_the_status_flag(path):
    """An all-zero inequality block (stored entries, all 0.0) whose right-hand side is violated: the direction meets no column,
    the reference's IndexError."""
    from pysparselp_amd.DualGradientAscent import STATUS_EMPTY, dual_gradient_ascent, exact_dual_line_search

    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = dga_args(load_golden("lp_sc50a"))
    empty = scipy.sparse.csr_matrix((np.zeros(6), np.array([0, 5, 1, 7, 2, 9]), np.array([0, 2, 4, 6])), shape=(3, c.size))
    assert empty.nnz == 6
    with pytest.raises(ValueError, match="empty breakpoint set"):
        exact_dual_line_search(np.array([-1.0, -2.0, 0.0]), empty, np.ones(3), c, ub, lb, path=path)
    state, mat = device_state((c, a_eq, b_eq, empty, np.ones(3), lb, ub), path)   # 0 - 1 < 0 on every inequality row
    try:
        state.iterate(1)
        assert state.status()[0] & STATUS_EMPTY
        with pytest.raises(ValueError, match="empty breakpoint set"):
            state.check()
    finally:
        state.close()
        mat.close()
    with pytest.raises(ValueError, match="empty breakpoint set"):
        dual_gradient_ascent(None, LP(c, a_eq, b_eq, empty, np.ones(3), lb, ub), nb_max_iter=5)
