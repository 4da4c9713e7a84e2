"""Host side of compaction for dual gradient ascent on a list (``slp_many_dual_set_compaction`` / ``slp_many_dual_live_state``,
``DeviceDGAMany.set_compaction`` / ``live_state``, ``dual_gradient_ascent_many_compact``, ``solve_dga_many_compact``): the two
prototypes are in a header of their own and bound in a table of their own while slp_hip.h, its 215 entry points, the other
extension headers and the existing Python signatures stay; the new functions take the arguments of the ``_cutoff`` forms and make
their refusals, before the library is touched.  None of it needs a GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import pysparselp_amd
from conftest import REPO, load_golden, lp_from_golden
from dga_many_cases import LP
from pysparselp_amd import _lib
from pysparselp_amd.DualGradientAscent import DeviceDGAMany
from pysparselp_amd.SparseLP import SparseLP
from test_cp_many_stop_host import BAD_EVERY, BAD_TOL, no_library  # noqa: F401
from test_dga_many_stop_host import fifteen

NEW = ["slp_many_dual_live_state", "slp_many_dual_set_compaction"]
HEADER = "slp_hip_ext_dga_many_live.h"


def _strip(text):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


# ------------------------------------------------------------------ header, bindings, signatures
def test_the_two_prototypes_are_in_a_header_of_their_own_and_bound():
    include = os.path.join(REPO, "include")
    assert f'#include "{HEADER}"' in open(os.path.join(include, "slp_hip_ext.h")).read()
    ext = _strip(open(os.path.join(include, HEADER)).read())
    assert "int slp_many_dual_set_compaction(slp_many_dga *s, int on);" in ext
    assert "int slp_many_dual_live_state(slp_many_dga *s, int64_t *live, int32_t *order, int64_t *launched, int64_t *cap);" in ext
    declared = sorted(set(re.findall(r"\b(slp_[a-z0-9_]+)\s*\(", ext)))
    assert declared == sorted(_lib.EXT_DGA_MANY_LIVE_SYMBOLS) == NEW
    assert _lib.EXT_DGA_MANY_LIVE_SYMBOLS == tuple(_lib._EXT_DGA_MANY_LIVE_SIGNATURES)
    # ... and in no other header; slp_hip.h keeps its 215 entry points, slp_hip_ext_dga_many.h its two
    for other in sorted(os.listdir(include)):
        if other != HEADER:
            text = _strip(open(os.path.join(include, other)).read())
            assert not any(name in text for name in NEW), other
    assert len(_lib.EXPORTED_SYMBOLS) == 215
    many = _strip(open(os.path.join(include, "slp_hip_ext_dga_many.h")).read())
    assert sorted(set(re.findall(r"\b(slp_[a-z0-9_]+)\s*\(", many))) == sorted(_lib.EXT_DGA_MANY_SYMBOLS)
    assert len(_lib.EXT_DGA_MANY_SYMBOLS) == 2
    others = (_lib.EXPORTED_SYMBOLS, _lib.EXT_SYMBOLS, _lib.EXT_ADMM_BATCH_SYMBOLS, _lib.EXT_DGA_BATCH_SYMBOLS, _lib.EXT_DGA_MANY_SYMBOLS,
              _lib.EXT_TALL_SYMBOLS)
    lib = _lib.load()   # dlopen works without a GPU
    for name in NEW:
        assert hasattr(lib, name), name
        for table in others:
            assert name not in table, name
    assert lib.slp_many_dual_set_compaction.argtypes == [_lib.c_vp, _lib.c_int]
    assert lib.slp_many_dual_live_state.argtypes == [_lib.c_vp] * 5
    assert lib.slp_many_dual_set_compaction.restype is _lib.c_int and lib.slp_many_dual_live_state.restype is _lib.c_int
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "C ABI (215 entry points)" in readme and HEADER in readme
    assert all(name in readme for name in NEW) and "dual_gradient_ascent_many_compact" in readme and "solve_dga_many_compact" in readme
    makefile = open(os.path.join(REPO, "pysparselp_amd", "csrc", "Makefile")).read()
    assert makefile.count("../../include/" + HEADER) == 2   # both dependency lists


def test_names_and_signatures():
    from pysparselp_amd import (dual_gradient_ascent_many_compact, dual_gradient_ascent_many_cutoff, solve_dga_many_compact,
                                solve_dga_many_cutoff)

    for name in ("dual_gradient_ascent_many_compact", "solve_dga_many_compact"):
        assert name in pysparselp_amd.__all__ and hasattr(pysparselp_amd, name) and name in pysparselp_amd.__doc__, name
    assert len(set(pysparselp_amd.__all__)) == len(pysparselp_amd.__all__)
    assert str(inspect.signature(dual_gradient_ascent_many_compact)) == (
        "(lps, tol, check_every=10, nb_max_iter=1000, callback_func=None, y_eq=None, y_ineq=None, max_time=None, targets=None)")
    assert str(inspect.signature(solve_dga_many_compact)) == (
        "(lps, tol, check_every=10, get_timing=True, nb_iter=10000, max_time=None, targets=None)")
    assert pysparselp_amd.SparseLP.solve_dga_many_compact is solve_dga_many_compact
    # the arguments of the forms with cut-offs, which keep theirs
    assert inspect.signature(dual_gradient_ascent_many_compact) == inspect.signature(dual_gradient_ascent_many_cutoff)
    assert inspect.signature(solve_dga_many_compact) == inspect.signature(solve_dga_many_cutoff)
    assert str(inspect.signature(DeviceDGAMany.set_compaction)) == "(self, on=True)"
    assert str(inspect.signature(DeviceDGAMany.live_state)) == "(self)"
    assert str(inspect.signature(DeviceDGAMany.set_cutoff)) == "(self, tol, check_every=1, targets=None)"


# ------------------------------------------------------------------ refusals before the library: those of the _cutoff forms
def _refusal(call):
    """The type and the text of what ``call`` raises."""
    with pytest.raises(Exception) as caught:
        call()
    return type(caught.value), str(caught.value)


def test_bad_arguments_are_refused_before_the_library_as_the_cutoff_forms_refuse_them(no_library):  # noqa: F811
    from pysparselp_amd import (dual_gradient_ascent_many_compact, dual_gradient_ascent_many_cutoff, solve_dga_many_compact,
                                solve_dga_many_cutoff)

    lps = [LP(*args) for args in fifteen()[:2]]
    golden = [lp_from_golden(load_golden("lp_potts8"), SparseLP)]
    bad = [((None,), {}), ((-1.0,), {}), ((1e-3,), {"targets": [0.0, 1.0, 2.0]}), ((1e-3,), {"targets": "1.0"}), ((1e-3,), {"targets": [True, False]}),
           ((1e-3,), {"targets": np.zeros((2, 1))})]
    bad += [((None,), {"targets": t}) for t in (np.nan, -np.inf, [0.0, np.nan], [0.0, -np.inf])]
    bad += [((tol,), {"targets": 0.0}) for tol in BAD_TOL if tol is not None]
    bad += [((None, every), {"targets": 0.0}) for every in BAD_EVERY]
    bad += [((1e-3, every), {}) for every in BAD_EVERY]
    seen = set()
    for args, kw in bad:
        for new, old, problems in ((dual_gradient_ascent_many_compact, dual_gradient_ascent_many_cutoff, lps),
                                   (solve_dga_many_compact, solve_dga_many_cutoff, golden)):
            if problems is golden and np.ndim(kw.get("targets", 0.0)) == 1 and len(kw["targets"]) == 2:
                kw = dict(kw, targets=kw["targets"][1:])   # one LP in that list
            want = _refusal(lambda: old(problems, *args, **kw))
            assert want[0] is ValueError, (args, kw, want)
            assert _refusal(lambda: new(problems, *args, **kw)) == want, (args, kw)
            seen.add(want[1][:24])
    assert len(seen) >= 5   # "both are None", NaN or -inf, the shape of targets, tol, check_every
    for new, old in ((dual_gradient_ascent_many_compact, dual_gradient_ascent_many_cutoff), (solve_dga_many_compact, solve_dga_many_cutoff)):
        want = _refusal(lambda: old([], None, targets=0.0))
        assert want[0] is ValueError and "empty list" in want[1]
        assert _refusal(lambda: new([], None, targets=0.0)) == want
    with pytest.raises(ValueError, match="lps must be a sequence"):
        dual_gradient_ascent_many_compact(5, 1e-3)


def test_an_accepted_call_gets_as_far_as_the_library(no_library):  # noqa: F811
    from pysparselp_amd import dual_gradient_ascent_many_compact, solve_dga_many_compact

    lps = [LP(*args) for args in fifteen()[:2]]
    with pytest.raises(AssertionError, match="library was loaded"):
        dual_gradient_ascent_many_compact(lps, None, 1, nb_max_iter=3, targets=[0.0, np.inf])
    with pytest.raises(AssertionError, match="library was loaded"):
        dual_gradient_ascent_many_compact(lps, 1e-3, nb_max_iter=3)
    with pytest.raises(AssertionError, match="library was loaded"):
        solve_dga_many_compact([lp_from_golden(load_golden("lp_potts8"), SparseLP)], 1e-3, nb_iter=3, targets=5)


def test_set_compaction_takes_a_switch_only():
    state = DeviceDGAMany.__new__(DeviceDGAMany)   # no handle: the check comes before the library
    for bad in (2, -1, "on", None, 0.5):
        with pytest.raises(ValueError, match="on must be True or False"):
            state.set_compaction(bad)
    state._h = None   # nothing to destroy
