"""Host side of compaction for the Chambolle-Pock and the ADMM list solver (``slp_many_cp_set_compaction`` /
``slp_many_cp_live_state``, ``slp_many_admm_set_compaction`` / ``slp_many_admm_live_state``; ``CPManyState`` /
``ADMMManyState.set_compaction`` / ``live_state``): the four prototypes are in a header of their own and bound in a table of
their own while slp_hip.h, its 215 entry points, the other extension headers, the other tables and the arguments of the existing
Python functions stay.  None of it needs a GPU."""
import inspect
import os
import re

import pytest

import pysparselp_amd
from conftest import REPO
from pysparselp_amd import ADMMManyState, CPManyState, _lib

NEW = ["slp_many_admm_live_state", "slp_many_admm_set_compaction", "slp_many_cp_live_state", "slp_many_cp_set_compaction"]
HEADER = "slp_hip_ext_many_live.h"


def _strip(text):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_the_four_prototypes_are_in_a_header_of_their_own_and_bound():
    include = os.path.join(REPO, "include")
    assert f'#include "{HEADER}"' in open(os.path.join(include, "slp_hip_ext.h")).read()
    ext = _strip(open(os.path.join(include, HEADER)).read())
    for solver, handle in (("cp", "slp_cp_many"), ("admm", "slp_admm_many")):
        assert f"int slp_many_{solver}_set_compaction({handle} *s, int on);" in ext
        assert (f"int slp_many_{solver}_live_state({handle} *s, int64_t live[2], int32_t *order, int64_t launched[2], int64_t cap[2]);"
                in ext)
    declared = sorted(set(re.findall(r"\b(slp_[a-z0-9_]+)\s*\(", ext)))
    assert declared == sorted(_lib.EXT_MANY_LIVE_SYMBOLS) == NEW
    assert _lib.EXT_MANY_LIVE_SYMBOLS == tuple(_lib._EXT_MANY_LIVE_SIGNATURES)
    for other in sorted(os.listdir(include)):   # ... and in no other header
        if other != HEADER:
            text = _strip(open(os.path.join(include, other)).read())
            assert not any(name in text for name in NEW), other
    assert len(_lib.EXPORTED_SYMBOLS) == 215
    others = (_lib.EXPORTED_SYMBOLS, _lib.EXT_SYMBOLS, _lib.EXT_ADMM_BATCH_SYMBOLS, _lib.EXT_DGA_BATCH_SYMBOLS, _lib.EXT_DGA_MANY_SYMBOLS,
              _lib.EXT_DGA_MANY_LIVE_SYMBOLS, _lib.EXT_TALL_SYMBOLS)
    lib = _lib.load()   # dlopen works without a GPU
    for name in NEW:
        assert hasattr(lib, name), name
        assert all(name not in table for table in others), name
        fn = getattr(lib, name)
        assert fn.restype is _lib.c_int
        assert fn.argtypes == ([_lib.c_vp, _lib.c_int] if name.endswith("set_compaction") else [_lib.c_vp] * 5)
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "C ABI (215 entry points)" in readme and HEADER in readme and all(name in readme for name in NEW)
    makefile = open(os.path.join(REPO, "pysparselp_amd", "csrc", "Makefile")).read()
    assert makefile.count("../../include/" + HEADER) == 2   # both dependency lists


def test_the_states_have_the_two_methods():
    for cls in (CPManyState, ADMMManyState):
        assert str(inspect.signature(cls.set_compaction)) == "(self, on=True)"
        assert str(inspect.signature(cls.live_state)) == "(self)"
        assert "read" in cls.set_compaction.__doc__ and "synchronises" in cls.set_compaction.__doc__   # the sync a call begins with
    assert (CPManyState._LIVE, ADMMManyState._LIVE) == ("slp_many_cp", "slp_many_admm")
    # a switch on the state: no function name was added
    assert not [name for name in pysparselp_amd.__all__ if "compact" in name and "dga" not in name and "dual_gradient" not in name]
    assert "set_compaction" in pysparselp_amd.__doc__


def test_set_compaction_takes_a_switch_only():
    for cls in (CPManyState, ADMMManyState):
        state = cls.__new__(cls)   # no handle: the check comes before the library
        for bad in (2, -1, "on", None, 0.5):
            with pytest.raises(ValueError, match="on must be True or False"):
                state.set_compaction(bad)
        state._h = None   # nothing to destroy
