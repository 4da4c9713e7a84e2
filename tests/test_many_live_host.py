"""The chunk plan of the live list of the list solvers and the launch cap of a call that runs over it (``csrc/slp_many_plan.h``:
``many_live_per``, ``many_live_range``, ``many_live_count``, ``many_live_write``, ``many_live_cap`` -- the text ``k_many_live`` of
``csrc/slp_many.h`` and ``slp_many_dga_iterate`` compile), on the CPU: a stand-alone program (``tests/host/many_live_main.cpp``) is
built with the host compiler under AddressSanitizer and UBSan and run as a child process, as ``test_many_plan_host.py`` does.
Nothing is loaded into Python."""
import os
import subprocess

from conftest import REPO


def test_the_live_list_tiles_the_lps_and_the_cap_follows_the_live_count(tmp_path):
    exe = str(tmp_path / "many_live_main")
    cxx = os.environ.get("CXX", "g++")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            "-I", os.path.join(REPO, "pysparselp_amd", "csrc"), os.path.join(REPO, "tests", "host", "many_live_main.cpp"),
                            "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok:") and " 0 failures" in run.stdout
    assert run.stderr == ""
