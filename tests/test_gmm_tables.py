"""CPU test of the launch geometry and buffer sizes of medgp_gmm_fit (medgp_amd/csrc/gmm_tables.h): the stand-alone program
gmm_tables_test.cpp checks them against restatements.  It is built with the host compiler under -fsanitize=address,undefined and
started as an ordinary child process: a mistake in this host arithmetic would otherwise be an out-of-bounds access on the GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medgp_amd", "csrc")


def test_gmm_geometry_under_sanitizers():
    subprocess.check_call(["make", "-s", "-C", CSRC, "gmm_tables_test"])
    out = subprocess.run([os.path.join(CSRC, "gmm_tables_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "gmm_tables ok" in out.stdout
