#!/usr/bin/env python3
"""Writes fixed_effects_parent.npz: every array the calls of tests/fixed_effects_cases.py return (statuses among them).  Keys:
"<family>/<case>/<call>/n" (number of returned arrays) and "<family>/<case>/<call>/<i>" (array i, dtype and shape kept; beta_cov at
64 columns included in full: the whole fixture stays far below the 1 MiB the project allows a committed file, which the script checks).
Run by hand on an MI355X with the library of the commit BEFORE k_mean_small / k_basis_small and k_mean_post / k_basis_post were put
on shared bodies (a checkout of that commit, or MEDGP_LIB=<that build>):

    python tests/golden/make_fixed_effects_parent.py [output.npz]

Every case is run twice, each time on a fresh context; the script stops without writing if the two runs differ in any byte, or if
a case does not return the statuses it claims.  tests/test_fixed_effects_bits_gpu.py demands these bits of every later library.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import fixed_effects_cases as FC  # noqa: E402


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "fixed_effects_parent.npz")
    for k in ("MEDGP_WGRAD_DEEP", "MEDGP_LA_PARK", "MEDGP_V0", "MEDGP_NO_CLASSES", "MEDGP_DEBUG_FAIL_ATTEMPTS", "MEDGP_MULTI_CU", "MEDGP_CHOLINV_NW"):
        os.environ.pop(k, None)
    out, unstable = {}, []
    for fam, cid in FC.CASES:
        first, second = FC.run(fam, cid), FC.run(fam, cid)
        want = FC.setup(fam, cid)["status"]
        for call in FC.CALLS:
            (arrs, st), (arrs2, _) = first[call], second[call]
            same = len(arrs) == len(arrs2) and all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(arrs, arrs2))
            if not same:
                unstable.append(f"{fam}/{cid}/{call}")
            if "marginal" in call:
                assert list(st) == want, (fam, cid, call, list(st))
            key = f"{fam}/{cid}/{call}/"
            out[key + "n"] = np.array(len(arrs), dtype=np.int64)
            for i, a in enumerate(arrs):
                out[key + str(i)] = np.ascontiguousarray(a)
            print(key, "status", np.asarray(st).tolist(), "arrays", len(arrs), "stable" if same else "UNSTABLE", flush=True)
    if unstable:
        sys.exit(f"not run-to-run stable, nothing written: {unstable}")
    np.savez_compressed(dst, **out)
    size = os.path.getsize(dst)
    print("wrote", dst, size, "bytes")
    if size >= 1 << 20:
        os.remove(dst)
        sys.exit("the fixture would pass 1 MiB: nothing kept")


if __name__ == "__main__":
    main()
