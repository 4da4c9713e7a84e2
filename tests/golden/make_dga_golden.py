"""Fixtures for dual gradient ascent (reference DualGradientAscent.py:36-245): what the reference returns on the LPs of the other
fixtures, a few of its line-search calls, and its two recorded dual_gradient_ascent curves.  Build container only:

    python tests/golden/make_dga_golden.py      -> tests/golden/dga.npz, tests/golden/ref_dga_curves.json

dga.npz holds, per case: `<case>_it` the iterations kept; `<case>_x`, `<case>_yeq`, `<case>_yineq` what the reference returns
after it + 1 iterations (x of the top of iteration it, the multipliers after it); `<case>_draws` the tie draws it has taken by
then; `<case>_horizon` the last kept iteration up to which tests/dga_cpu.py in every re-ordered form (blocked scans of 16, 64 and
256 elements, the device's own order) equals the reference bit for bit; and captured calls of exact_dual_line_search:
`<case>_ls_it`, `_ls_kind` (0 inequality rows, 1 equality rows), `_ls_g_ineq` / `_ls_g_eq` (the directions, in call order per
kind), `_ls_cbar`, `_ls_step`, `_ls_draw` (the uniform draw a tie took, else NaN).  The LPs are the fixtures' own
(lp_<name>.npz).  While generating, dga_cpu(order="reference") is asserted equal to the imported reference bit for bit.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import make_golden  # noqa: E402

SMALL = [0, 1, 10, 100, 1000]
KEEP = {"sc50a": SMALL, "potts8": SMALL, "random0": SMALL, "random1": SMALL, "random2": SMALL,
        "sc105": [0, 1, 10, 50, 100, 150, 200, 300], "potts50": [0, 1, 10, 100, 200, 300]}
REQUIRED = {"sc50a": 1000, "potts8": 1000, "random0": 1000, "random1": 1000, "random2": 1000, "sc105": 100, "potts50": 200}
LS_DEFAULT = (0, 1, 10, 100)   # iterations whose line-search calls are kept
LS_AT = {"potts50": (0, 10)}


class _LP:
    pass


def lp_of(d):
    import scipy.sparse

    def csr(tag):
        shape = tuple(int(v) for v in d[f"{tag}_shape"])
        return scipy.sparse.csr_matrix((d[f"{tag}_data"], d[f"{tag}_indices"], d[f"{tag}_indptr"]), shape=shape)

    lp = _LP()
    lp.costsvector, lp.lower_bounds, lp.upper_bounds = d["c"].copy(), d["lb"].copy(), d["ub"].copy()
    lp.a_equalities, lp.b_equalities = csr("Ae"), d["be"].copy()
    ai = csr("Ai")
    lp.a_inequalities = ai if ai.shape[0] > 0 else None
    lp.b_upper = d["bu"].copy()
    lp.b_lower = None if bool(d["bl_none"]) else d["bl"].copy()
    return lp


def main():
    make_golden.build_reference()
    make_golden.install_shims()
    import pysparselp.DualGradientAscent as ref
    from dga_cpu import dga_cpu

    sink = io.StringIO()
    out = {}
    ties_inside = 0
    for name, keep in KEEP.items():
        lp = lp_of(dict(np.load(os.path.join(HERE, f"lp_{name}.npz"))))
        args = (lp.costsvector, lp.a_equalities, lp.b_equalities, lp.a_inequalities, lp.b_upper, lp.lower_bounds, lp.upper_bounds)
        last = max(keep)
        mine = dga_cpu(*args, nb_max_iter=last + 1, order="reference", keep=keep)
        # the reference, once per kept iteration (it returns only its last state); tie draws counted at numpy's generator
        draws = [0]
        rand = np.random.rand

        def counted(*shape):
            if not shape:
                draws[0] += 1
            return rand(*shape)

        xs, yes, yis, nd = [], [], [], []
        np.random.rand = counted
        try:
            for it in keep:
                draws[0] = 0
                with contextlib.redirect_stdout(sink):
                    x, y_eq, y_ineq = ref.dual_gradient_ascent(None, lp, nb_max_iter=it + 1, max_time=None)
                mx, mye, myi, mnd = mine[it]
                assert np.array_equal(x, mx) and np.array_equal(y_eq, mye) and draws[0] == mnd, (name, it)
                assert (y_ineq is None and myi is None) or np.array_equal(y_ineq, myi), (name, it)
                xs.append(x); yes.append(y_eq); yis.append(np.zeros(0) if y_ineq is None else y_ineq); nd.append(draws[0])
        finally:
            np.random.rand = rand
        # the re-ordered forms: how far do they all stay on the reference's bits
        horizon = last
        for order, block in (("blocked", 16), ("blocked", 64), ("blocked", 256), ("device", 0)):
            try:
                other = dga_cpu(*args, nb_max_iter=last + 1, order=order, block=block, keep=keep)
            except (AssertionError, ValueError):
                other = {}
            ok = -1
            for it in keep:
                if it not in other:
                    break
                same = all(np.array_equal(p, q) for p, q in zip(other[it][:2], mine[it][:2])) and other[it][3] == mine[it][3]
                same = same and (mine[it][2] is None or np.array_equal(other[it][2], mine[it][2]))
                if not same:
                    break
                ok = it
            horizon = min(horizon, ok)
        assert horizon >= REQUIRED[name], (name, horizon)
        # a handful of line-search calls (the restatement equals the reference bit for bit: its calls are the reference's)
        calls = []
        wanted = [it for it in LS_AT.get(name, LS_DEFAULT) if it <= horizon]

        def on_search(it, kind, g, c_bar, step, draw, calls=calls, wanted=wanted):
            if it in wanted:
                calls.append((it, kind, g.copy(), c_bar.copy(), step, draw))

        dga_cpu(*args, nb_max_iter=max(wanted) + 1, order="reference", on_search=on_search)
        out[f"{name}_it"] = np.array(keep)
        out[f"{name}_x"] = np.array(xs)
        out[f"{name}_yeq"] = np.array(yes)
        out[f"{name}_yineq"] = np.array(yis)
        out[f"{name}_draws"] = np.array(nd)
        out[f"{name}_horizon"] = np.array(horizon)
        out[f"{name}_ls_it"] = np.array([c[0] for c in calls])
        out[f"{name}_ls_kind"] = np.array([0 if c[1] == "ineq" else 1 for c in calls])
        for kind in ("ineq", "eq"):   # directions in call order, per kind of rows (their lengths differ)
            gs = [c[2] for c in calls if c[1] == kind]
            out[f"{name}_ls_g_{kind}"] = np.array(gs) if gs else np.zeros((0, 0))
        out[f"{name}_ls_cbar"] = np.array([c[3] for c in calls])
        out[f"{name}_ls_step"] = np.array([c[4] for c in calls])
        out[f"{name}_ls_draw"] = np.array([c[5] for c in calls])
        inside = nd[keep.index(horizon)]
        ties_inside += inside > 0
        print(f"{name}: n={lp.costsvector.size}, horizon {horizon}, tie draws inside it {inside}, {len(calls)} line searches kept")
    assert ties_inside >= 3
    path = os.path.join(HERE, "dga.npz")
    np.savez_compressed(path, **out)
    print(f"dga.npz: {os.path.getsize(path) / 1e3:.0f} kB")
    curves = {}
    for f in ("netlib_curves_SC105.json", "test_pott_segmentation_curves.json"):
        curves[f] = json.load(open(os.path.join(make_golden.REF_SRC, "tests", f)))["dual_gradient_ascent"]
    json.dump(curves, open(os.path.join(HERE, "ref_dga_curves.json"), "w"))


if __name__ == "__main__":
    main()
