"""The window of tie draws that the three dual-gradient-ascent handles share (``csrc/slp_dga_draws.h``), on the CPU: a stand-alone
program with the hand-written cases (``tests/host/dga_draws_main.cpp``) is built with the host compiler -- the C++ driver of the
gcc the oracle is built with -- under AddressSanitizer and UBSan and run as a child process.  Nothing is loaded into Python."""
import os
import subprocess

from conftest import REPO


def test_the_draw_window_keeps_the_three_handles_rules(tmp_path):
    exe = str(tmp_path / "dga_draws_main")
    cxx = os.environ.get("CXX", "g++")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            "-I", os.path.join(REPO, "pysparselp_amd", "csrc"), os.path.join(REPO, "tests", "host", "dga_draws_main.cpp"),
                            "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok:") and " 0 failures" in run.stdout
    assert run.stderr == ""
