"""Writes tests/golden/time_shift_spread.json: what a legitimate fp64 program that forms its cosines from tables of cos / sin (w t)
loses in the fp64 outputs of the inference calls when the time axis moves to |t| = 2^10 and 2^14 h -- the errors of
time_shift_cases.tables_restate against the references, per (family, offset), in the scale of each quantity's existing bar.

Run by hand from the repository root after `make -C oracle`, never by the suite:

    python tests/golden/make_time_shift_spread.py

Uses the project's own code only (tests/time_shift_cases.py).  tests/test_time_shift.py re-derives the numbers and compares them with
the file; tests/test_time_shift_gpu.py takes the device's fp64 bounds at an offset from it.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import time_shift_cases as S  # noqa: E402


def main():
    spread = S.measure_spread()
    for name, rows in spread.items():
        for off, e in rows.items():
            print(f"{name:5s} offset {off:>7s}: " + "  ".join(f"{k} {e[k]:.2e}" for k in S.SPREAD_KEYS if k in e))
    doc = {"what": "worst error of time_shift_cases.tables_restate (fp64, cosine tables at the shifted times) against the references "
                   "of the unshifted inputs, per family and offset [h]; lpd relative to max(1, |ref|), loo_obj / loo_grad as "
                   "nlml_truth.error_pair",
           "spread": spread}
    with open(S.GOLDEN, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", S.GOLDEN)


if __name__ == "__main__":
    main()
