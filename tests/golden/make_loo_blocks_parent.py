#!/usr/bin/env python3
"""Writes loo_blocks_parent.npz: every array the calls of tests/loo_blocks_cases.py return and the launch count of every profile
label, each call made on a fresh context.  Keys as in objective_calls_parent.npz: "labels" (the profile label names, once),
"<call>/counts" (int64, in the order of labels), "<call>/n" (number of returned arrays) and "<call>/<i>" (array i, dtype and shape
kept).  Run by hand on an MI355X with the library of the commit BEFORE the staged 64-column products and the block-column inverse were
folded onto panel_product / loo_block_column_inverse (a checkout of that commit, or MEDGP_LIB=<that build>):

    python tests/golden/make_loo_blocks_parent.py [output.npz]

Every call is made twice; the script stops without writing if the two runs differ in any byte or count.
tests/test_loo_blocks_bits_gpu.py demands these bits and counts of every later library.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import loo_blocks_cases as LB  # noqa: E402
import objective_calls_cases as OC  # noqa: E402


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "loo_blocks_parent.npz")
    for k in ("MEDGP_WGRAD_DEEP", "MEDGP_LA_PARK", "MEDGP_V0", "MEDGP_NO_CLASSES", "MEDGP_DEBUG_FAIL_ATTEMPTS", "MEDGP_MULTI_CU", "MEDGP_CHOLINV_NW"):
        os.environ.pop(k, None)
    out, labels, unstable = {}, None, []
    first, second = LB.run_fresh(), LB.run_fresh()
    for cname, (arrs, counts, res, plan) in first.items():
        arrs2, counts2, _, plan2 = second[cname]
        assert plan == plan2 == OC.PLAN[LB.FAM], (cname, plan)
        if labels is None:
            labels = sorted(counts)
        same = counts == counts2 and len(arrs) == len(arrs2) and all(
            a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(arrs, arrs2))
        if not same:
            unstable.append(cname)
        key = cname + "/"
        out[key + "counts"] = np.array([counts[k] for k in labels], dtype=np.int64)
        out[key + "n"] = np.array(len(arrs), dtype=np.int64)
        for i, a in enumerate(arrs):
            out[key + str(i)] = np.ascontiguousarray(a)
        print(key, "status", np.asarray(LB.statuses(cname, res)).tolist(), "launches", {k: v for k, v in counts.items() if v}, "arrays", len(arrs),
              "stable" if same else "UNSTABLE", flush=True)
    if unstable:
        sys.exit(f"not run-to-run stable, nothing written: {unstable}")
    out["labels"] = np.array(labels)
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
