"""The scalar rule that repairs an ADMM multiplier for the duality-gap certificate (``csrc/slp_admm_gap.h``), on the CPU: the
one text the kernels of ``slp_admm.hip`` and ``slp_admm_cg.hip`` compile, built into a stand-alone program
(``tests/host/admm_gap_dual_main.cpp``) with the host compiler under AddressSanitizer and UBSan, ``-ffp-contract=off`` as the
library, and run as a child process, as ``test_cp_gap_decide_host.py`` does.  The program reads the table this test writes --
signed zeros, infinities, NaN and denormals in every position -- and prints bits; they are compared with
``admm_gap_cpu.scalar_rule``.  Nothing is loaded into Python."""
import itertools
import os
import struct
import subprocess

import numpy as np

import admm_gap_cpu
from conftest import REPO

INF, NAN, TINY = np.inf, np.nan, 5e-324


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _cases():
    a = [0.0, -0.0, 1.0, -1.0, -0.7071067811865476, INF, -INF, NAN, TINY, -TINY]
    lam = [0.0, -0.0, 2.5, -2.5, INF, -INF, NAN, TINY, -TINY, 1e308]
    boxes = [(-INF, 1.5), (-1.5, INF), (-INF, INF), (-2.0, 3.0), (0.0, 0.0), (-0.0, 0.0), (-INF, 0.0), (0.0, INF), (NAN, 1.0), (-INF, NAN),
             (-INF, -TINY), (TINY, INF)]
    return [(x, y, lo, hi) for x, y, (lo, hi) in itertools.product(a, lam, boxes)]


def test_the_table_reaches_every_answer():
    got = [admm_gap_cpu.scalar_rule(*case) for case in _cases()]
    assert any(r for r, _ in got) and any(not r for r, _ in got)
    # the slack of an inequality row a x - s = 0, s <= bu (its entry negative after scaling): a negative multiplier gives the slack
    # a positive cost and pushes it down, where it has no bound
    assert admm_gap_cpu.scalar_rule(-0.7, -2.5, -INF, 1.5) == (True, 0.0)
    assert admm_gap_cpu.scalar_rule(-0.7, 2.5, -INF, 1.5) == (False, 2.5)
    assert admm_gap_cpu.scalar_rule(-0.7, 0.0, -INF, 1.5) == (False, 0.0)
    assert admm_gap_cpu.scalar_rule(TINY, TINY, -INF, INF) == (False, TINY)        # the product underflows to 0: no term at all
    repaired, y = admm_gap_cpu.scalar_rule(1.0, NAN, -INF, INF)
    assert not repaired and np.isnan(y)                                             # a NaN is not hidden by the repair


def test_the_rule_of_the_kernels_under_the_host_compiler(tmp_path):
    exe, path = str(tmp_path / "admm_gap_dual_main"), str(tmp_path / "cases.txt")
    cxx = os.environ.get("CXX", "g++")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            "-I", os.path.join(REPO, "pysparselp_amd", "csrc"), os.path.join(REPO, "tests", "host", "admm_gap_dual_main.cpp"),
                            "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    cases = _cases()
    with open(path, "w") as f:
        for case in cases:
            f.write(" ".join("%016x" % _bits(v) for v in case) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == ""
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok: %d cases" % len(cases) and len(lines) == len(cases) + 1
    wrong = []
    for case, line in zip(cases, lines):
        flag, ybits = line.split()
        repaired, y = admm_gap_cpu.scalar_rule(*case)
        got = struct.unpack("<d", struct.pack("<Q", int(ybits, 16)))[0]
        same = np.isnan(got) if np.isnan(y) else int(ybits, 16) == _bits(y)
        if int(flag) != int(repaired) or not same:
            wrong.append((case, (repaired, y), line))
    assert not wrong, wrong[:10]
