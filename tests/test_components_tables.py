"""CPU test of the tile builder of medgp_components_batch (build_components_tiles, medgp_amd/csrc/inference_tables.h): the stand-alone
program components_tables_test.cpp checks it against a brute-force restatement for Q in {1, 2, 3, 5, 17, 64}, point counts 0, 1,
tile - 1, tile, tile + 1 and several tiles, under budgets from "everything in one chunk" to "one tile per chunk".  It is built with
the host compiler under -fsanitize=address,undefined and started as an ordinary child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medgp_amd", "csrc")


def test_components_tile_builder_against_brute_force_under_sanitizers():
    subprocess.check_call(["make", "-s", "-C", CSRC, "components_tables_test"])
    out = subprocess.run([os.path.join(CSRC, "components_tables_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "components_tables ok" in out.stdout
