"""What keeps tests/test_gpu_fuzz_batched.py from passing vacuously, checked without a GPU on the generators and CPU references of
tools/fuzz_batched.py with the GPU test's own seed and case count: the dual-ascent LPs mostly run clean, some raise each of the
two line-search errors in a way the device can be compared with, the horizons are worth comparing,
HiGHS solves every clean one, and the Chambolle-Pock / ADMM LPs are accepted by the entry points and reach the wave, tile and
padding sizes they are drawn for.  For tests/test_gpu_fuzz_many_stop.py: under the drawn tolerances, by the numpy restatements
alone, stopping and running LPs stand side by side in the lists -- in the long one, at every cadence, at the large sizes, warm and
cold, with equality rows only -- the chosen LP mostly stops by exact equality, and one Chambolle-Pock list stops at a step of 0.0.
For tests/test_gpu_fuzz_cp_gap.py: boxing an LP changes its bounds and nothing else; the certificate's lists and batches have a
finite bound at every edge size, hold stopping and running LPs of every kind, unbounded LPs and boxed LPs that never stop, and
almost no undecidable check; HiGHS solves every LP or calls it unbounded, and the restatement's own bounds are lower bounds by
HiGHS and agree with the formula in exact rational arithmetic.  For tests/test_gpu_fuzz_admm_batch_stop.py: the batches reach every
edge size and the sizes 1, 65 and 260, hold stopping and running instances side by side, tiles that hold both and tiles that
are wholly stopped early under the drawn width and under 64, per-instance bounds and starts, and share their references; and
the draws of the families that were there before are what they were."""
import os
import sys

import numpy as np
import scipy.sparse

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_batched  # noqa: E402

SEED, CASES = fuzz_batched.TEST_SEED, fuzz_batched.TEST_CASES


def _pool():
    return [lp for batch in fuzz_batched.dga_pool(CASES, SEED) for lp in batch]


def test_dga_lps_mostly_run_clean_and_some_raise_each_error():
    stats = fuzz_batched.dga_statistics(CASES, SEED)
    for kind, s in stats.items():
        print(f"{kind}: {s['clean']} clean / {s['no_crossing']} no-crossing / {s['empty']} empty / {s['negative']} negative step of "
              f"{s['drawn']}; {s['comparable_raises']} raises comparable on the device; shortest horizon of a clean LP {s['min_horizon']}")
        assert s["drawn"] >= CASES // 2 and 2 * s["clean"] >= s["drawn"], kind
    assert sum(s["no_crossing"] for s in stats.values()) >= 1 and sum(s["empty"] for s in stats.values()) >= 1
    comparable = {lp.fail[1] for lp in _pool() if lp.status_ok}
    assert {"never changes sign", "empty breakpoint set"} <= comparable
    # a raise in a later iteration with clean LPs around it: the status checks compare iterates before and after it
    assert any(lp.status_ok and lp.fail[0] > 0 for lp in _pool())
    # dga_cpu in the device's own order runs clean wherever the reference's order does: the device must then end without a flag,
    # and the GPU test asserts that no dual bound went unchecked
    assert all(lp.device_fail is None for lp in _pool() if lp.clean)
    for kind in ("integer", "decimal"):   # every kind meets every edge size; some LPs take tie draws, at different counts
        assert set(fuzz_batched.EDGE_N) <= {lp.args[0].size for lp in _pool()}
        draws = {lp.states[fuzz_batched.DGA_ITERS - 1][3] for lp in _pool() if lp.kind == kind and lp.clean}
        print(f"{kind}: tie draws taken after {fuzz_batched.DGA_ITERS} iterations: {sorted(draws)}")
    assert len({lp.states[fuzz_batched.DGA_ITERS - 1][3] for lp in _pool() if lp.clean}) >= 3
    assert fuzz_batched.DGA_TILE_EDGE in [len(batch) for batch in fuzz_batched.dga_pool(CASES, SEED)]
    assert max(len(lps) for lps in fuzz_batched.dga_lists(CASES, SEED)) > 256


def test_dga_lps_have_a_horizon_worth_comparing():
    """The horizon -- how far dga_cpu agrees with itself in its three orders -- is the full run on the decimal-valued clean LPs
    and falls below 10 iterations on at most one clean LP in ten of either kind (integer-valued: equal breakpoints, which the
    reference's unstable sort and the device's stable one order differently)."""
    for kind in ("integer", "decimal"):
        clean = [lp for lp in _pool() if lp.kind == kind and lp.clean]
        short = [lp.name for lp in clean if lp.horizon < 10]
        full = sum(lp.horizon == fuzz_batched.DGA_ITERS - 1 for lp in clean)
        print(f"{kind}: {len(clean)} clean, {full} with the full horizon, horizons {sorted({lp.horizon for lp in clean})}, below 10: {len(short)}")
        late = sum(len(lp.late_stops()) for lp in clean)
        print(f"{kind}: {late} comparisons behind the horizon, with dga_cpu in the device's order")
        assert 10 * len(short) <= len(clean) and 2 * full >= len(clean), kind
    for lp in _pool():   # only the compared prefix is shortened: no LP with a complete iteration is left out
        assert lp.stops() == sorted({s for s in fuzz_batched.DGA_STOPS if s <= lp.horizon} | ({lp.horizon} if lp.horizon >= 0 else set()))
        assert all(s in lp.states for s in lp.stops())


def test_dga_lps_meet_the_solvers_preconditions_and_highs_solves_the_clean_ones():
    from pysparselp_amd.DualGradientAscent import FUSED_MAX

    for lp in _pool():
        c, a_eq, b_eq, a_ineq, b_upper, lb, ub = lp.args
        assert 1 <= c.size <= FUSED_MAX and sum(lp.rows) >= 1, lp.name
        assert np.all(np.isfinite(lb)) and np.all(np.isfinite(ub)) and np.all(lb <= ub), lp.name
        if lp.kind == "integer":
            for v in (c, lb, ub, b_eq, a_eq.data) + (() if a_ineq is None else (b_upper, a_ineq.data)):
                assert np.array_equal(v, np.round(v)), lp.name
            assert np.all(a_eq.data != 0) and (a_ineq is None or np.all(a_ineq.data != 0))
        if lp.clean:
            assert lp.linprog().status == 0, (lp.name, lp.linprog().message)
    assert any(np.any(lp.args[5] == lp.args[6]) for lp in _pool())
    assert any(np.any(lp.args[0] == 0) for lp in _pool())


def _finite_side_per_row(problem):
    _, _, _, a_ineq, bl, bu, _, _ = problem
    if a_ineq is None:
        return True
    bu, bl = np.atleast_2d(bu), (None if bl is None else np.atleast_2d(bl))
    return bool(np.all(np.isfinite(bu) | (False if bl is None else np.isfinite(bl))))


def _shape_facts(lps):
    """(the n that occur, the longest row, an empty row?, an empty column over both blocks?)"""
    ns, longest, empty_row, empty_col = set(), 0, False, False
    for lp in lps:
        n = lp["c"].shape[-1]
        ns.add(n)
        blocks = [a for a in (lp["a_eq"], lp["a_ineq"]) if a is not None]
        longest = max([longest] + [int(np.diff(a.indptr).max()) for a in blocks if a.shape[0]])
        empty_row = empty_row or any(np.any(np.diff(a.indptr) == 0) for a in blocks)
        used = np.zeros(n, dtype=bool)
        for a in blocks:
            used[a.indices] = True
            assert np.all(a.data != 0)
        empty_col = empty_col or not used.all()
    return ns, longest, empty_row, empty_col


def test_cp_and_admm_lps_pass_validation_and_reach_the_edge_sizes():
    from pysparselp_amd.ADMM import _validate_batch
    from pysparselp_amd.ChambollePockPPD import _many_problem, one_sided_system_batch

    cp_batches = fuzz_batched.cp_batch_cases(CASES, SEED)
    admm_batches = fuzz_batched.admm_batch_cases(CASES, SEED)
    lists = fuzz_batched.cp_many_cases(CASES, SEED)
    for args, its, plot in cp_batches:
        assert 1 <= its <= 60 and plot in fuzz_batched.CADENCES
        if args["a_ineq"] is not None:   # the pattern of finite sides is that of instance 0 in every instance
            mat, b = one_sided_system_batch(args["a_ineq"], args["b_lower"], args["b_upper"])
            assert b.shape[-1] == mat[3]
        for k in range(args["c"].shape[0]):
            problem, x0 = fuzz_batched.of_instance(args, k)
            _many_problem(k, problem)
            assert _finite_side_per_row(problem) and np.all(problem[6] <= problem[7])
    for args, its, plot in admm_batches:
        assert args["a_ineq"] is not None and np.all(np.isfinite(args["c"]))
        _validate_batch(args["c"], args["a_eq"], args["beq"], args["a_ineq"], args["b_lower"], args["b_upper"], args["lb"], args["ub"], args["x0"])
        assert _finite_side_per_row(fuzz_batched.of_instance(args, 0)[0])
    for lps, its, plot in lists:
        for k, lp in enumerate({id(lp): lp for lp in lps}.values()):
            _many_problem(k, fuzz_batched.of_instance(lp, 0)[0])
            assert _finite_side_per_row(fuzz_batched.of_instance(lp, 0)[0])
    assert fuzz_batched.CP_TILE_EDGE in [a["c"].shape[0] for a, _, _ in cp_batches]
    assert fuzz_batched.ADMM_TILE_EDGE in [a["c"].shape[0] for a, _, _ in admm_batches]
    assert max(len(lps) for lps, _, _ in lists) > 256 and {len(lps) for lps, _, _ in lists} >= {1, 2, 3}
    everything = [a for a, _, _ in cp_batches] + [a for a, _, _ in admm_batches] + [lp for lps, _, _ in lists for lp in lps]
    ns, longest, empty_row, empty_col = _shape_facts(everything)
    print("n drawn:", sorted(ns), "longest row:", longest)
    assert set(fuzz_batched.EDGE_N) <= ns and longest > 64 and empty_row and empty_col
    for name, family in (("cp_batch", [a for a, _, _ in cp_batches]), ("admm_batch", [a for a, _, _ in admm_batches]),
                         ("cp_many", [lp for lps, _, _ in lists for lp in lps])):
        ns, longest, empty_row, empty_col = _shape_facts(family)
        print(name, "edge n drawn:", sorted(ns & set(fuzz_batched.EDGE_N)), "longest row:", longest)
        assert longest > 64 and empty_row and empty_col and set(fuzz_batched.EDGE_N) <= ns, name
        assert any(np.any(lp["lb"] == lp["ub"]) for lp in family) and any(np.any(np.isinf(lp["lb"])) for lp in family), name
        assert any(lp["x0"] is not None for lp in family) and any(lp["x0"] is None for lp in family), name
        assert any(lp["b_lower"] is not None for lp in family) and any(lp["b_lower"] is None for lp in family), name
    assert any(a["a_ineq"] is None for a, _, _ in cp_batches) and any(lp["a_ineq"] is None for lps, _, _ in lists for lp in lps)
    assert any(a["a_eq"] is None for a, _, _ in cp_batches) and any(a["a_eq"] is not None for a, _, _ in cp_batches)
    assert any(a["b_upper"] is not None and a["b_upper"].ndim == 2 for a, _, _ in cp_batches)   # per-instance right-hand sides
    assert any(a["lb"].ndim == 2 for a, _, _ in cp_batches) and any(a["lb"].ndim == 2 for a, _, _ in admm_batches)


# ---- the per-LP stopping lists: what keeps tests/test_gpu_fuzz_many_stop.py from passing vacuously -------------------------------------

def _stop_facts(cases):
    """Per list ``dict(case, every, exact, early, tol, entries)`` from the restatement alone; ``entries``: one ``(stopped, n, warm,
    equalities only, step)`` per LP of the list."""
    out = []
    for case in cases:
        want = case.want()
        iterations, stopped, step = want[0], want[1], want[-1]
        entries = [(bool(stopped[k]), lp["c"].size, lp["x0"] is not None, lp["a_ineq"] is None, float(step[k])) for k, lp in enumerate(case.lps)]
        k = case.k_star
        out.append(dict(case=case, every=case.every, tol=case.tol, entries=entries, exact=bool(stopped[k]) and iterations[k] == case.t_star,
                        early=bool(stopped[k]) and iterations[k] < case.t_star))
        assert all(iterations[~stopped] == case.total) and all(iterations[stopped] % case.every == 0)
        assert stopped[k] and iterations[k] <= case.t_star   # the LP the tolerances come from meets them at t_star at the latest
    return out


def _both(entries):
    """Does a set of entries hold a stopping and a running LP?"""
    kinds = {e[0] for e in entries}
    return kinds == {True, False}


def _assert_stop_conditions(family, cases):
    from pysparselp_amd import _many

    facts = _stop_facts(cases)
    assert len(facts) == CASES
    for f in facts:   # the draws: the horizon, the cadences, a check iteration in the last two thirds, tolerances the entry points take
        case = f["case"]
        assert case.total == 20 + case.its and case.every in (1, 3, 10) and 0 <= case.k_star < len(case.lps)
        assert case.t_star % case.every == 0 and case.total // 3 <= case.t_star <= case.total
        assert 1 <= case.after <= max(1, case.total // 3 - 1)
        for tol in case.tol:
            assert _many.check_stop(tol, case.every) == (tol, case.every)
    everything = [e for f in facts for e in f["entries"]]
    short = [e for f in facts if len(f["entries"]) <= 256 for e in f["entries"]]
    long_lists = [f["entries"] for f in facts if len(f["entries"]) > 256]
    stopping = [e for e in everything if e[0]]
    large = [e for e in everything if e[1] >= 127]
    print(f"{family}: {len(stopping)} of {len(everything)} list entries stop; without the long list {sum(e[0] for e in short)} of {len(short)}; "
          f"{sum(_both(f['entries']) for f in facts)} of {len(facts)} lists hold both kinds; k_star stops exactly at t_star in "
          f"{sum(f['exact'] for f in facts)} lists, earlier in {sum(f['early'] for f in facts)}; n >= 127: {sum(e[0] for e in large)} stop, "
          f"{sum(not e[0] for e in large)} run; the long list: {[sum(e[0] for e in entries) for entries in long_lists]} of "
          f"{[len(entries) for entries in long_lists]} stop; equalities only: {sum(e[0] and e[3] for e in everything)} stop, "
          f"{sum(e[3] and not e[0] for e in everything)} run; tol == 0.0 in cases {[i for i, f in enumerate(facts) if f['tol'][-1] == 0.0]}")
    for entries in (everything, short):
        assert 4 * sum(e[0] for e in entries) >= len(entries) and 4 * sum(not e[0] for e in entries) >= len(entries)
    assert 2 * sum(_both(f["entries"]) for f in facts) >= len(facts)
    assert sum(f["exact"] for f in facts) >= 8 and sum(f["early"] for f in facts) >= 1
    for every in (1, 3, 10):
        assert _both([e for f in facts if f["every"] == every for e in f["entries"]]), every
    assert _both(large)
    assert {e[2] for e in stopping} == {True, False}
    assert len(long_lists) == 1 and _both(long_lists[0])
    return facts, everything


def test_admm_stopping_lists_hold_stopping_and_running_lps_of_every_kind():
    _assert_stop_conditions("admm", fuzz_batched.admm_stop_cases(CASES, SEED))


def test_cp_stopping_lists_hold_stopping_and_running_lps_of_every_kind():
    facts, everything = _assert_stop_conditions("cp", fuzz_batched.cp_stop_cases(CASES, SEED))
    assert _both([e for e in everything if e[3]])   # among the LPs with equality rows only
    # an exact fixed point: a tolerance of 0.0 under which an LP stops at a step of exactly 0.0
    assert any(f["tol"] == (0.0,) and any(e[0] and e[4] == 0.0 for e in f["entries"]) for f in facts)


# ---- the certified stopping test: what keeps tests/test_gpu_fuzz_cp_gap.py from passing vacuously -------------------------------------

def test_a_boxed_lp_is_the_same_lp_with_its_finite_bounds():
    """``random_lp(..., boxed=True)`` consumes the draws of ``boxed=False``: from equal generator states the two LPs differ in
    ``lb`` / ``ub`` only -- there only where the unboxed one is infinite -- and leave the generator in the same state."""
    infinite = 0
    for family in ("cp", "admm", "dga"):
        for seed, n in ((1, None), (2, 65), (3, 1), (4, 257), (5, None), (6, 2)):
            plain_rng, boxed_rng = np.random.RandomState(seed), np.random.RandomState(seed)
            plain, boxed = fuzz_batched.random_lp(plain_rng, family, n), fuzz_batched.random_lp(boxed_rng, family, n, boxed=True)
            for a, b in zip(plain_rng.get_state(), boxed_rng.get_state()):
                assert np.array_equal(a, b)
            assert sorted(plain) == sorted(boxed)
            for name in plain:
                p, b = plain[name], boxed[name]
                if name in ("lb", "ub"):
                    assert np.all(np.isfinite(b)) and np.array_equal(p[np.isfinite(p)], b[np.isfinite(p)]), (family, seed, name)
                    infinite += int(np.isinf(p).sum())
                elif p is None or b is None:
                    assert p is None and b is None, (family, seed, name)
                elif scipy.sparse.issparse(p):
                    assert p.shape == b.shape and (p != b).nnz == 0, (family, seed, name)
                else:
                    assert np.array_equal(p, b), (family, seed, name)
            assert np.all(boxed["lb"] <= boxed["ub"])
    assert infinite > 0


def _gap_lp_shape(problem):
    """(n, the longest row, an empty row?, an empty column over both blocks?) of an 8-tuple."""
    blocks = [a for a in (problem[1], problem[3]) if a is not None and a.shape[0]]
    n = problem[0].size
    used = np.zeros(n, dtype=bool)
    for a in blocks:
        used[a.indices] = True
    return (n, max(int(np.diff(a.indptr).max()) for a in blocks), any(np.any(np.diff(a.indptr) == 0) for a in blocks), not used.all())


def _assert_gap_conditions(family, cases, large):
    """(a) .. (f) of the certificate's randomised cases, on the restatement alone.  ``large``: the number of entries of the long
    list / the tile-edge batch.  Returns the statistics."""
    import cp_gap_cpu

    assert len(cases) == CASES
    stats = fuzz_batched.gap_statistics(cases)
    print(family, stats)
    entries, shapes, highs_checked = [], [], 0
    for no, case in enumerate(cases):
        want, keep = case.want(), case.keep()
        assert case.total == fuzz_batched.STOP_EXTRA + case.its and case.every in fuzz_batched.STOP_EVERY
        assert case.t_star % case.every == 0 and case.total // 3 <= case.t_star <= case.total
        assert 1 <= case.after <= max(1, case.total // 3 - 1)
        assert all(want[0][~want[1]] == case.total) and all(want[0][want[1]] % case.every == 0)
        if case.k_star is None:
            assert case.tol == fuzz_batched.NEVER_TOL and not any(ref.finite_checks(case.every, case.total, case.t_star) for ref in case.entries)
        else:   # (d) the LP the tolerances come from meets them at t_star at the latest, and its check there is decidable
            star = case.entries[case.k_star]
            assert case.tol[1] == star.cert.violation[case.t_star - 1]
            assert cp_gap_cpu.decidable(star.cert, case.t_star, *case.tol), no
            assert cp_gap_cpu.decision(star.cert.primal[case.t_star - 1], star.cert.bound[case.t_star - 1], star.cert.violation[case.t_star - 1], *case.tol)
            assert want[1][case.k_star] and want[0][case.k_star] <= case.t_star, no
        entries += [(bool(want[1][k]), ref.n, ref.warm, ref.eq_only, case.every, len(case.entries)) for k, ref in enumerate(case.entries)]
        for ref in case.distinct():
            if ref.finite_checks(case.every, case.total):   # (a)
                shapes.append(_gap_lp_shape(ref.problem))
            res, cert = ref.highs(), ref.cert
            stops = [bool(want[1][k]) for k, other in enumerate(case.entries) if other is ref]
            assert res.status in (0, 3), (no, res.status, res.message)   # (e)
            if res.status == 3:
                assert np.all(np.isneginf(cert.bound)) and not any(stops), no
                continue
            finite = np.isfinite(cert.bound)
            assert np.all(cert.bound[finite] <= res.fun + fuzz_batched.gap_highs_slack(cert.band[finite], res.fun)), no
            highs_checked += int(finite.sum())
            if any(stops):
                t = int(want[0][[other is ref for other in case.entries].index(True)])
                if cert.violation[t - 1] == 0.0:
                    assert cert.primal[t - 1] >= res.fun - fuzz_batched.gap_highs_slack(cert.band[t - 1], res.fun), no
        done = {}
        for k, (ref, record) in enumerate(zip(case.entries, fuzz_batched.gap_final_records(case))):   # (f)
            if record is not None and (id(ref), record[0]) not in done:
                kind = fuzz_batched.gap_bound_kind(record[1].bound, fuzz_batched.gap_exact_bound(ref, record[2]), record[1].band)
                assert kind is not None, (no, k, record[1])
                done[(id(ref), record[0])] = kind
    # (a)
    ns = {s[0] for s in shapes}
    print(family, "with a finite bound at a check: n", sorted(ns), "longest row", max(s[1] for s in shapes))
    assert set(fuzz_batched.EDGE_N) <= ns and max(s[1] for s in shapes) > 64 and any(s[2] for s in shapes) and any(s[3] for s in shapes)
    # (b)
    assert stats["entries"] == len(entries) and stats["stopped"] == sum(e[0] for e in entries)
    assert 4 * stats["stopped"] >= stats["entries"] and 4 * stats["running"] >= stats["entries"]
    assert large in [e[5] for e in entries] and _both([e for e in entries if e[5] == large])
    for every in fuzz_batched.STOP_EVERY:
        assert _both([e for e in entries if e[4] == every]), every
    assert _both([e for e in entries if e[1] >= 127])
    assert _both([e for e in entries if e[2]]) and _both([e for e in entries if not e[2]]) and _both([e for e in entries if e[3]])
    # (c)
    assert stats["unbounded"] >= 1 and stats["boxed_never"] >= 1
    # (d)
    assert stats["left_out"] <= fuzz_batched.GAP_LEFT_OUT * stats["entries"]
    assert stats["left_out_late"] <= fuzz_batched.GAP_LEFT_OUT * stats["entries"]
    # (e): the allowance for HiGHS's own tolerances is ten times the measured excess, at least 1e-9
    assert highs_checked == stats["finite_records"] > 0
    assert fuzz_batched.HIGHS_ALLOWANCE >= max(10 * stats["highs_excess"], fuzz_batched.ENERGY_TOL["rtol"])
    return stats


def test_cp_list_certificate_cases_hold_what_the_gpu_test_claims():
    stats = _assert_gap_conditions("cp_many_gap", fuzz_batched.cp_gap_cases(CASES, SEED), fuzz_batched.LONG_LIST)
    assert stats["rounded_to_zero"] == fuzz_batched.CP_GAP_ROUNDED_TO_ZERO


def test_cp_batch_certificate_cases_hold_what_the_gpu_test_claims():
    stats = _assert_gap_conditions("cp_batch_gap", fuzz_batched.cp_batch_gap_cases(CASES, SEED), fuzz_batched.CP_TILE_EDGE)
    assert stats["rounded_to_zero"] == fuzz_batched.CP_BATCH_GAP_ROUNDED_TO_ZERO


# ---- the batched ADMM stopping test: what keeps tests/test_gpu_fuzz_admm_batch_stop.py from passing vacuously -------------------------

def test_admm_batch_stopping_cases_hold_what_the_gpu_test_claims():
    import time

    from pysparselp_amd import _many
    from pysparselp_amd.ADMM import _validate_batch

    fuzz_batched._STOP_CASES.pop(("admm_batch", CASES, SEED), None)
    start = time.perf_counter()
    cases = fuzz_batched.admm_batch_stop_cases(CASES, SEED)
    elapsed = time.perf_counter() - start
    assert len(cases) == CASES and elapsed < 30, elapsed   # the references are shared by the cycled instances
    sizes = [len(case.lps) for case in cases]
    assert [case.args["c"].shape[1] for case in cases[:len(fuzz_batched.EDGE_N)]] == list(fuzz_batched.EDGE_N)
    assert {1, 65, fuzz_batched.LONG_LIST} <= set(sizes) and sizes[fuzz_batched.large_case(CASES)] == fuzz_batched.LONG_LIST
    assert set(sizes) <= set(fuzz_batched.ADMM_BATCH_STOP_SIZES) | {fuzz_batched.LONG_LIST}
    both = spread = stopped = running = 0
    tiles = {"drawn": [0, 0], "64": [0, 0]}
    stops = []
    for case in cases:
        a, want = case.args, case.want()
        _validate_batch(a["c"], a["a_eq"], a["beq"], a["a_ineq"], a["b_lower"], a["b_upper"], a["lb"], a["ub"], a["x0"])
        assert case.distinct() == min(len(case.lps), fuzz_batched.ADMM_BATCH_DISTINCT) == case.distinct_args["c"].shape[0]
        assert all(case.ref(k) is case.ref(k % case.distinct()) for k in range(len(case.lps)))
        assert case.total == fuzz_batched.STOP_EXTRA + case.its and case.every in fuzz_batched.STOP_EVERY and case.plot in fuzz_batched.CADENCES
        assert case.t_star % case.every == 0 and case.total // 3 <= case.t_star <= case.total and 0 <= case.k_star < len(case.lps)
        assert 1 <= case.after <= max(1, case.total // 3 - 1) and case.width in fuzz_batched.ADMM_BATCH_WIDTHS
        assert 1 <= case.rearm < case.t_star and case.rearm < case.off <= case.total
        assert case.rearm % case.every == 0 or case.t_star == case.every   # a check, where one lies before t_star
        for tol in case.tol:
            assert _many.check_stop(tol, case.every) == (tol, case.every)
        assert case.tol == tuple(float(curve[case.t_star - 1]) for curve in case.ref(case.k_star).curves)
        assert want[1][case.k_star] and want[0][case.k_star] <= case.t_star   # the instance the tolerances come from stops by then
        assert all(want[0][~want[1]] == case.total) and all(want[0][want[1]] % case.every == 0)
        for col, dtype in zip(want, (np.int64, bool, np.float64, np.float64)):
            assert col.dtype == dtype and col.shape == (len(case.lps),)
        stopped += int(want[1].sum())
        running += int((~want[1]).sum())
        both += bool(want[1].any() and not want[1].all())
        spread += len(set(want[0][want[1]])) >= 3
        stops += list(want[0][want[1]])
        for name, width in (("drawn", case.width), ("64", 64)):
            mixed, dead = fuzz_batched.stop_tiles(want, width, case.every)
            tiles[name][0] += mixed
            tiles[name][1] += dead
    print(f"admm_batch_stop: {sum(sizes)} instances, {stopped} stop and {running} run; {both} of {CASES} batches hold both kinds, {spread} stop at "
          f"three or more distinct iterations; stopping iterations {min(stops)} .. {max(stops)}; (mixed, dead) tiles {tiles}; restated in {elapsed:.1f} s")
    assert 3 * both >= CASES and spread >= 1
    assert all(count >= 1 for pair in tiles.values() for count in pair), tiles
    # a levels launch with several workgroups along x and several tiles: more than 256 (row, instance) lanes in the widest pass
    assert any(case.ref(0).xs[0].size * case.width > 256 and len(case.lps) > case.width for case in cases)
    lps = [case.distinct_args for case in cases]
    ns, longest, empty_row, empty_col = _shape_facts(lps)
    assert set(fuzz_batched.EDGE_N) <= ns and longest > 64 and empty_row and empty_col
    assert any(np.ndim(lp["lb"]) == 2 for lp in lps) and any(np.ndim(lp["x0"]) == 2 for lp in lps)
    assert any(np.any(np.isinf(lp["lb"])) for lp in lps) and any(np.any(lp["lb"] == lp["ub"]) for lp in lps)


def test_stop_tiles_on_hand_made_states():
    want = (np.array([10, 20, 40, 40, 10, 10, 40, 30]), np.array([True, True, False, False, True, True, False, True]))
    assert fuzz_batched.stop_tiles(want, 2, 10) == (1, 2)   # tiles (10, 20) and (10, 10) are dead, (40 running, 30) is mixed
    assert fuzz_batched.stop_tiles(want, 4, 10) == (2, 0)
    assert fuzz_batched.stop_tiles(want, 8, 10) == (1, 0)
    all_stop = (np.array([10, 10, 20, 25]), np.ones(4, dtype=bool))
    assert fuzz_batched.stop_tiles(all_stop, 2, 10) == (0, 1)   # the first tile stops a check before the second one
    assert fuzz_batched.stop_tiles(all_stop, 2, 20) == (0, 0) and fuzz_batched.stop_tiles(all_stop, 64, 1) == (0, 0)
    assert fuzz_batched.stop_tiles(want, 1, 10)[0] == 0


def _digest(cases):
    """sha256 over everything a family's generator returns: every array with type and shape, every matrix, every number."""
    import hashlib

    h = hashlib.sha256()

    def feed(v):
        if isinstance(v, dict):
            for key in sorted(v):
                h.update(key.encode())
                feed(v[key])
        elif isinstance(v, (list, tuple)):
            h.update(b"[%d" % len(v))
            for item in v:
                feed(item)
        elif scipy.sparse.issparse(v):
            v = v.tocsr()
            feed([np.asarray(v.shape), v.indptr.astype(np.int64), v.indices.astype(np.int64), v.data])
        elif v is None:
            h.update(b"None")
        elif isinstance(v, np.ndarray):
            h.update(str((v.dtype.str, v.shape)).encode())
            h.update(np.ascontiguousarray(v).tobytes())
        else:
            h.update(repr(v).encode())

    feed(cases)
    return h.hexdigest()


def test_the_draws_of_the_existing_families_are_untouched():
    """The digests of the commit before the batched ADMM stopping family, for ``TEST_SEED`` / ``TEST_CASES``."""
    before = {"admm_batch_cases": "e65595c8598c6fd2d14050914a6fa807284bda09e397da13fbd0af0935d717e5",
              "admm_many_cases": "86591dc894861a5331138b20bab4d3f874d413a3dafecb1d0b261eda73b1eb48",
              "cp_batch_cases": "3fbf0c7742a276a6472c421c6e13af765b46e5a1dd2341eb4fcef457c8fff750"}
    fuzz_batched.admm_batch_stop_cases(CASES, SEED)   # drawing the new family changes none of them
    for name, digest in before.items():
        assert _digest(getattr(fuzz_batched, name)(CASES, SEED)) == digest, name
