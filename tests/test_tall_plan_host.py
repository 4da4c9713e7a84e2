"""The geometry planner of the tall-cell format (``csrc/slp_tall_plan.h``: rows per block, strip width, capacity of the value
table and the LDS layout of the product kernel), on the CPU: a stand-alone program (``tests/host/tall_plan_main.cpp``) sweeps
shapes, densities, dictionaries, switches and chunkings, compares the geometry with a strip-range split against a copy of the
code the planner replaced and pins the benchmark's LP (config 4) at R = 13 021, C = 3 072 in both orientations -- A through the
chunk rule with 96 row blocks per chunk, not 11 161 / 3 584.  It is built with the host compiler under AddressSanitizer and
UBSan and run as a child process, as ``test_many_plan_host.py`` does.  Nothing is loaded into Python."""
import os
import subprocess

from conftest import REPO


def test_the_planner_of_the_tall_cells_keeps_its_rules(tmp_path):
    exe = str(tmp_path / "tall_plan_main")
    cxx = os.environ.get("CXX", "g++")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            "-I", os.path.join(REPO, "pysparselp_amd", "csrc"), os.path.join(REPO, "tests", "host", "tall_plan_main.cpp"),
                            "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "config 4: A^T R 13021 C 3072" in run.stdout and "; A R 13021 C 3072" in run.stdout and "(96 per chunk)" in run.stdout
    assert run.stdout.splitlines()[-1].startswith("ok:") and " 0 failures" in run.stdout
    assert run.stderr == ""
