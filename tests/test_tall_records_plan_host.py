"""The planner's choice between the two packet forms of a tall-cell copy (``csrc/slp_tall_plan.h``: ``tall_plan_records``), on the
CPU: a stand-alone program (``tests/host/tall_records_plan_main.cpp``) is built with the host compiler under AddressSanitizer and
UBSan and run as a child process, as ``test_tall_packet_host.py`` does.  Nothing is loaded into Python.

Checked there: the benchmark's LP (BASELINE config 4) plans records in both orientations and in every one of its 16 chunks, through
the carry, at R = 13 021 and C = 3 072 as before; the 60 000 x 300 000 LP at 2e-4 in 8 chunks plans slot-major; over a sweep of
shapes, densities, dictionaries, forced geometries and strip-range splits a plan says records exactly where the growth predicted for
its cell -- worked out in the test from the format's description -- is at most 1/16, for items with a value id; items with an fp64
value stay slot-major whatever the growth (measured 10 % slower with records: DESIGN section 3 (ix));
``SLP_TALL_RECORDS`` forces either form; a carried form overrides the chunk's own rule."""
import os
import subprocess

from conftest import REPO


def test_records_are_planned_where_the_copy_grows_by_at_most_a_sixteenth(tmp_path):
    exe = str(tmp_path / "tall_records_plan_main")
    cxx = os.environ.get("CXX", "g++")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            "-I", os.path.join(REPO, "pysparselp_amd", "csrc"), os.path.join(REPO, "tests", "host", "tall_records_plan_main.cpp"),
                            "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ok:" in run.stdout and " 0 failures" in run.stdout
    assert run.stderr == ""
