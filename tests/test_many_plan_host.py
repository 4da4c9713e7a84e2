"""The launch planner that the three list solvers share (``csrc/slp_many_plan.h``: switches, forms, workgroup width, launch cap and
the check of a CSR block), on the CPU: a stand-alone program with the hand-written cases (``tests/host/many_plan_main.cpp``) is
built with the host compiler under AddressSanitizer and UBSan and run as a child process, as ``test_dga_draws_host.py`` does.
Nothing is loaded into Python."""
import os
import subprocess

from conftest import REPO


def test_the_planner_of_the_list_solvers_keeps_its_rules(tmp_path):
    exe = str(tmp_path / "many_plan_main")
    cxx = os.environ.get("CXX", "g++")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            "-I", os.path.join(REPO, "pysparselp_amd", "csrc"), os.path.join(REPO, "tests", "host", "many_plan_main.cpp"),
                            "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok:") and " 0 failures" in run.stdout
    assert run.stderr == ""
