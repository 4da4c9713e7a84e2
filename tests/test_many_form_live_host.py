"""What a compacted call of the Chambolle-Pock and the ADMM list solver is made of (``csrc/slp_many_plan.h``: the predicate
``ManyFormLive`` -- LP k has form g and is not stopped -- and ``many_form_call``, per form the live count and the launch cap;
the text ``cpm_run`` and ``admmm_run`` compile), on the CPU: a stand-alone program (``tests/host/many_form_live_main.cpp``) is
built with the host compiler under AddressSanitizer and UBSan and run as a child process, as ``test_many_live_host.py`` does.
Nothing is loaded into Python."""
import os
import subprocess

from conftest import REPO


def test_the_live_count_and_the_cap_per_form_are_those_of_a_plain_loop(tmp_path):
    exe = str(tmp_path / "many_form_live_main")
    cxx = os.environ.get("CXX", "g++")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            "-I", os.path.join(REPO, "pysparselp_amd", "csrc"),
                            os.path.join(REPO, "tests", "host", "many_form_live_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok:") and " 0 failures" in run.stdout
    assert run.stderr == ""
