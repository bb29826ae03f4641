"""CPU test of the plan of a call (medgp_amd/csrc/call_plan.h): the stand-alone program call_plan_test.cpp checks the route rule (the
round-4 thresholds of uniform calls, the plan of the heavy-tailed cohort of DESIGN 4.9, the one-entry route of medgp_get_factor), the
layout of size classes, memory waves and arena offsets, the look-ahead scratch layout, the chunks of medgp_screen and the grid of
k_wgrad against brute-force restatements.  It is built with the host compiler under -fsanitize=address,undefined and started as an
ordinary child process; the cohort's sizes (synth.ragged_sizes(0, 300)) are its arguments."""
import os
import subprocess

from medgp_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medgp_amd", "csrc")


def test_call_plan_against_brute_force_under_sanitizers():
    subprocess.check_call(["make", "-s", "-C", CSRC, "call_plan_test"])
    sizes = [str(int(n)) for n in synth.ragged_sizes(0, 300)]
    out = subprocess.run([os.path.join(CSRC, "call_plan_test")] + sizes, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "call_plan ok (cohort of 300 sizes)" in out.stdout
