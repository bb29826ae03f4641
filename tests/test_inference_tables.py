"""CPU test of the launch-table builders of the inference entry points (medgp_amd/csrc/inference_tables.h): the stand-alone program
inference_tables_test.cpp checks them against brute-force restatements.  It is built with the host compiler under
-fsanitize=address,undefined and started as an ordinary child process: an index mistake in this host arithmetic would otherwise be
an out-of-bounds access on the GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medgp_amd", "csrc")


def test_table_builders_against_brute_force_under_sanitizers():
    subprocess.check_call(["make", "-s", "-C", CSRC, "inference_tables_test"])
    out = subprocess.run([os.path.join(CSRC, "inference_tables_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "inference_tables ok" in out.stdout
