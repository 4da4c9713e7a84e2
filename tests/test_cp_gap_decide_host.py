"""The scalar arithmetic of the duality-gap certificate (``csrc/slp_cp_gap.h``: the NaN-propagating max and min, the column
and row terms of the bound with their guards, the violation fold and the decision with its finiteness rule), on the CPU: the one
text the kernels of ``slp_cp_many.hip`` and ``slp_cp_batch.hip`` compile, built into a stand-alone program
(``tests/host/cp_gap_decide_main.cpp``) with the host compiler under AddressSanitizer and UBSan, ``-ffp-contract=off`` as the
library, and run as a child process, as ``test_tall_plan_host.py`` does.  The program reads the cases this test writes and
prints bits; they are compared with ``cp_gap_cpu.decision`` and with the terms as ``cp_gap_cpu.Restatement.at`` forms them.
Nothing is loaded into Python."""
import os
import struct
import subprocess

import numpy as np

import cp_gap_cpu
from conftest import REPO

INF, NAN = np.inf, np.nan


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _same(got_bits, want):
    """Bit for bit, except that any NaN answers a NaN."""
    got = struct.unpack("<d", struct.pack("<Q", got_bits))[0]
    return np.isnan(got) if np.isnan(want) else got_bits == _bits(want)


def _fold(a, b, pick):
    """np.maximum / np.minimum, with the accumulator ``a`` kept on a tie (+0 against -0), as a lane's running value is."""
    with np.errstate(invalid="ignore"):
        want = float(pick(np.float64(a), np.float64(b)))
    return float(a) if want == a and not np.isnan(want) else want


def _cases():
    cases = []   # (operation, arguments, expected value or (bound, stop), what it is)
    edge = [NAN, 0.0, -0.0, INF, -INF, 1.0, -1.0]
    for a in edge:
        for b in edge:
            cases.append(("max", (a, b), _fold(a, b, np.maximum), "max"))
            cases.append(("min", (a, b), _fold(a, b, np.minimum), "min"))
    with np.errstate(invalid="ignore", over="ignore"):
        for d, lb, ub in [(0.0, -INF, 1.0), (-0.0, -INF, INF), (2.0, -INF, 3.0), (-2.0, -INF, 3.0), (0.5, -1.0, 3.0), (-0.5, -1.0, 3.0),
                          (NAN, 0.0, 1.0), (1.0, NAN, 1.0), (1.0, 0.0, NAN), (5e-324, -INF, INF)]:
            d_, lb_, ub_ = np.float64(d), np.float64(lb), np.float64(ub)
            cases.append(("col", (d, lb, ub), float(np.where(d_ != 0, np.minimum(d_ * lb_, d_ * ub_), 0.0)), "column term"))
        for y, b in [(0.0, INF), (-0.0, -INF), (2.0, 3.0), (-2.0, 3.0), (1.0, INF), (NAN, 1.0), (1.0, NAN), (0.0, NAN)]:
            y_, b_ = np.float64(y), np.float64(b)
            cases.append(("row", (y, b), float(np.where(y_ != 0, y_ * b_, 0.0)), "row term"))
        for so_far, v, eq in [(0.0, -3.0, 1.0), (0.0, -3.0, 0.0), (0.0, 3.0, 0.0), (4.0, -3.0, 1.0), (0.0, NAN, 1.0), (0.0, NAN, 0.0),
                              (NAN, 1.0, 0.0), (0.0, -INF, 1.0), (0.0, -INF, 0.0), (0.0, -0.0, 1.0)]:
            cases.append(("viol", (so_far, v, eq), _fold(so_far, abs(v) if eq else v, np.maximum), "violation"))
    below_half = float(np.nextafter(0.5, 0.0))
    decide = [
        # primal, cols, sy, violation, tol_gap, tol_feas
        ((1.0, 0.0, 0.0, 0.0, 0.5, 0.0), "gap equal to its threshold to the bit"),
        ((1.0, 0.0, 0.0, 0.0, below_half, 0.0), "gap one ulp above its threshold"),
        ((2.5, 3.0, 0.5, 0.0, 0.0, 0.0), "tol_gap 0 with gap 0"),
        ((2.5, 3.0, 0.5, 0.125, 0.0, 0.125), "violation equal to tol_feas"),
        ((2.5, 3.0, 0.5, float(np.nextafter(0.125, 1.0)), 0.0, 0.125), "violation one ulp above tol_feas"),
        ((1.0, -INF, 0.0, 0.0, 1e300, 1.0), "bound -inf from the columns"),
        ((1.0, 0.0, INF, 0.0, 1e300, 1.0), "bound -inf from the rows"),
        ((INF, INF, 0.0, 0.0, 1e300, 1.0), "primal = bound = +inf"),
        ((1.0, INF, INF, 0.0, 1e300, 1.0), "bound inf - inf"),
        ((1.0, 1.5, 0.25, 0.0, 1e-1, 0.0), "an ordinary stop"),
        ((1.0, 3.0, 0.25, 0.0, 1e-1, 0.0), "an ordinary go-on"),
    ]
    good = (2.5, 3.0, 0.5, 0.0, 1.0, 1.0)
    for k, name in enumerate(("primal", "cols", "sy", "violation", "tol_gap", "tol_feas")):
        decide.append((good[:k] + (NAN,) + good[k + 1:], "NaN in " + name))
    decide.append((good, "the same without a NaN"))
    with np.errstate(invalid="ignore"):
        for args, what in decide:
            primal, cols, sy, viol, tol_gap, tol_feas = (np.float64(v) for v in args)
            bound = float(cols - sy)
            cases.append(("decide", args, (bound, cp_gap_cpu.decision(float(primal), bound, float(viol), float(tol_gap), float(tol_feas))), what))
    return cases


def test_the_cases_are_what_they_claim():
    by_name = {what: (args, want) for op, args, want, what in _cases() if op == "decide"}
    (p, cols, sy, _, tol, _), (bound, stop) = by_name["gap equal to its threshold to the bit"]
    assert abs(p - bound) == tol * (1.0 + abs(p) + abs(bound)) and stop
    (p, cols, sy, _, tol, _), (bound, stop) = by_name["gap one ulp above its threshold"]
    assert abs(p - bound) == np.nextafter(tol * (1.0 + abs(p) + abs(bound)), INF) and not stop
    assert by_name["tol_gap 0 with gap 0"][1] == (2.5, True)
    assert by_name["violation equal to tol_feas"][1][1] and not by_name["violation one ulp above tol_feas"][1][1]
    assert by_name["bound -inf from the columns"][1] == (-INF, False) and by_name["bound -inf from the rows"][1] == (-INF, False)
    assert by_name["primal = bound = +inf"][1] == (INF, False)
    assert by_name["the same without a NaN"][1][1] and not any(want[1] for what, (_, want) in by_name.items() if what.startswith("NaN in "))
    assert by_name["an ordinary stop"][1][1] and not by_name["an ordinary go-on"][1][1]


def test_the_certificate_arithmetic_of_the_kernels_under_the_host_compiler(tmp_path):
    exe, path = str(tmp_path / "cp_gap_decide_main"), str(tmp_path / "cases.txt")
    cxx = os.environ.get("CXX", "g++")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            "-I", os.path.join(REPO, "pysparselp_amd", "csrc"), os.path.join(REPO, "tests", "host", "cp_gap_decide_main.cpp"),
                            "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    cases = _cases()
    with open(path, "w") as f:
        for op, args, _, _ in cases:
            f.write(op + "".join(" %016x" % _bits(a) for a in args) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == ""
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok: %d cases" % len(cases) and len(lines) == len(cases) + 1
    wrong = []
    for (op, args, want, what), line in zip(cases, lines):
        got = line.split()
        if op == "decide":
            ok = _same(int(got[0], 16), want[0]) and int(got[1]) == int(want[1])
        else:
            ok = _same(int(got[0], 16), want)
        if not ok:
            wrong.append((what, op, args, want, line))
    assert not wrong, wrong
