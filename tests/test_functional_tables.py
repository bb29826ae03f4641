"""CPU test of the host tables of medgp_functional_batch (check_functional_csr, functional_positions, build_functional_tiles,
medgp_amd/csrc/inference_tables.h): the stand-alone program functional_tables_test.cpp checks them against brute-force restatements
for functional counts 0, 1, 63, 64, 65 and several tiles, term counts 0, 1 and many, budgets from "everything in one chunk" to "one
tile per chunk", and broken offsets of every kind.  It is built with the host compiler under -fsanitize=address,undefined and started
as an ordinary child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medgp_amd", "csrc")


def test_functional_tables_against_brute_force_under_sanitizers():
    subprocess.check_call(["make", "-s", "-C", CSRC, "functional_tables_test"])
    out = subprocess.run([os.path.join(CSRC, "functional_tables_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "functional_tables ok" in out.stdout
