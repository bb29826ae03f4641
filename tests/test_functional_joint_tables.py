"""CPU test of the chunk builder of medgp_functional_joint_batch (build_functional_joint_chunks, medgp_amd/csrc/inference_tables.h):
the stand-alone program functional_joint_tables_test.cpp checks it against a brute-force restatement for functional counts 0, 1, 63,
64, 65, 130 and 200 per patient, budgets from "everything in one chunk" to "one patient per chunk", and the patient that alone exceeds
the budget: every patient once, every lower tile pair once, offsets inside the needs.  It is built with the host compiler under
-fsanitize=address,undefined and started as an ordinary child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medgp_amd", "csrc")


def test_functional_joint_tables_against_brute_force_under_sanitizers():
    subprocess.check_call(["make", "-s", "-C", CSRC, "functional_joint_tables_test"])
    out = subprocess.run([os.path.join(CSRC, "functional_joint_tables_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "functional_joint_tables ok" in out.stdout
