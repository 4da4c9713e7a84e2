"""The payload of a packet of the tall-cell format in its two forms -- slot-major, and the first four list positions as one
16-byte record per lane (``csrc/slp_tall_item.h``: ``tall_packet_layout`` and its companions, the one text for the builder, the
product kernel, the planner and this test), on the CPU: a stand-alone program (``tests/host/tall_packet_main.cpp``) is built with
the host compiler under AddressSanitizer and UBSan and run as a child process, as ``test_tall_item_host.py`` does.  Nothing is
loaded into Python.

Checked there, for both forms and both item kinds, on a host model of a cell (lists of 0-9 items over 1 024 lanes with widths that
are no multiple of 64; lists of 3 / 4 / 5 with a fifth-item slot one and two lanes wide; all lanes alike at 0, 4, 8 and 9; 20 random
non-increasing profiles): every item is found at the offset the kernel's formulas give (written out from the format's
description), every padding word is zero and lands in the scratch cell, every word is written once and read by exactly one lane,
and the cell's size is the sum of the per-lane sizes that the builder's scan, its estimate and the planner use."""
import os
import subprocess

from conftest import REPO


def test_both_packet_forms_are_written_and_read_at_the_same_offsets(tmp_path):
    exe = str(tmp_path / "tall_packet_main")
    cxx = os.environ.get("CXX", "g++")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            "-I", os.path.join(REPO, "pysparselp_amd", "csrc"), os.path.join(REPO, "tests", "host", "tall_packet_main.cpp"),
                            "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok:") and " 0 failures" in run.stdout
    assert run.stderr == ""
