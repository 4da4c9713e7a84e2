"""The stored item of the tall-cell format (``csrc/slp_tall_item.h``: the builder's packing and the product kernel's decoding to
LDS byte addresses, one text for both), on the CPU: a stand-alone program (``tests/host/tall_item_main.cpp``) is built with the
host compiler under AddressSanitizer and UBSan and run as a child process, as ``test_many_plan_host.py`` does.  Nothing is loaded
into Python.

Checked there: for every (value id, column, sum field) on the field boundaries and 10^5 random triples the decoding of the
encoding is the identity; the three byte addresses are 8 x index + base; the stored bits are those the format's description names;
the all-zero item is the scratch cell."""
import os
import subprocess

from conftest import REPO


def test_items_decode_to_the_byte_addresses_of_what_was_encoded(tmp_path):
    exe = str(tmp_path / "tall_item_main")
    cxx = os.environ.get("CXX", "g++")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            "-I", os.path.join(REPO, "pysparselp_amd", "csrc"), os.path.join(REPO, "tests", "host", "tall_item_main.cpp"),
                            "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok:") and " 0 failures" in run.stdout
    assert run.stderr == ""
