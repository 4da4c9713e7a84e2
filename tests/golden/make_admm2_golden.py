"""Fixtures for lp_admm2 (reference ADMM.py:272-474): iterates of the reference's lp_admm2, with its sparse LU of the KKT
matrix, on the LPs of the other fixtures, and the reference's recorded admm2 curves.  Build container only:

    python tests/golden/make_admm2_golden.py      -> tests/golden/admm2.npz, tests/golden/ref_admm2_curves.json

admm2.npz holds, per case, the iterations kept (`<case>_it`), the x the callback received there (`<case>_x`) and the
energy (`<case>_e1`).  The LPs are the fixtures' own (lp_<name>.npz, ka_l1svm.npz); `sc105_pre` is SC105 with
use_preconditioning=True.
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
import make_golden  # noqa: E402

KEEP = [0, 1, 10, 100, 200]
CASES = {"sc50a": "lp_sc50a", "sc105": "lp_sc105", "potts8": "lp_potts8", "potts50": "lp_potts50", "random0": "lp_random0",
         "random1": "lp_random1", "random2": "lp_random2", "l1svm": "ka_l1svm", "sc105_pre": "lp_sc105"}


def solver_args(d):
    import scipy.sparse

    def csr(tag):
        shape = tuple(int(v) for v in d[f"{tag}_shape"])
        m = scipy.sparse.csr_matrix((d[f"{tag}_data"], d[f"{tag}_indices"], d[f"{tag}_indptr"]), shape=shape)
        m.__dict__["blocks"] = []   # what the reference's modelling layer records (SparseLP.py:93-95)
        return m

    ae, ai = csr("Ae"), csr("Ai")
    bl = None if bool(d["bl_none"]) else d["bl"]
    a_eq, beq = (ae, d["be"]) if ae.shape[0] > 0 else (None, None)
    return d["c"], a_eq, beq, ai, bl, d["bu"], d["lb"], d["ub"]


def main():
    make_golden.build_reference()
    make_golden.install_shims()
    from pysparselp.ADMM import lp_admm2

    sink = io.StringIO()
    out = {}
    for name, fixture in CASES.items():
        d = dict(np.load(os.path.join(HERE, fixture + ".npz")))
        args = solver_args(d)
        with contextlib.redirect_stdout(sink):
            rec = make_golden.capture(lambda cb: lp_admm2(*args, nb_iter=200, nb_iter_plot=1, callback_func=cb, max_time=None,
                                                          use_preconditioning=name.endswith("_pre")), KEEP)
        assert rec["it"] == KEEP
        out[f"{name}_it"] = np.array(rec["it"])
        out[f"{name}_x"] = np.array(rec["x"])
        out[f"{name}_e1"] = np.array(rec["e1"])
        print(f"{name}: n={args[0].size}, energy at 200: {rec['e1'][-1]!r}")
    path = os.path.join(HERE, "admm2.npz")
    np.savez_compressed(path, **out)
    print(f"admm2.npz: {os.path.getsize(path) / 1e3:.0f} kB")
    curves = {}
    for f in ("netlib_curves_SC105.json", "test_pott_segmentation_curves.json"):
        curves[f] = json.load(open(os.path.join(make_golden.REF_SRC, "tests", f)))["admm2"]
    json.dump(curves, open(os.path.join(HERE, "ref_admm2_curves.json"), "w"))


if __name__ == "__main__":
    main()
