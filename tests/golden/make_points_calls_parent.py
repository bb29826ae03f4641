#!/usr/bin/env python3
"""Writes points_calls_parent.npz: every array the runs of tests/points_calls_cases.py return, the launch count of every profile label
and the plan of each run, each on a fresh context.  Keys: "labels" (the profile label names, once), "<family>/<budget>/<call>/counts"
(int64, in the order of labels), ".../plan" (int64 [classes, 2]), ".../n" (number of returned arrays) and ".../<i>" (array i, dtype and
shape kept).  Recorded once, by hand on an MI355X, from a checkout of the commit BEFORE the test-point handling of these calls was
folded onto shared helpers, with tests/points_calls_cases.py and this file copied in -- so with that commit's library AND its capi.py:

    python tests/golden/make_points_calls_parent.py [output.npz]

Every run is made twice; the script stops without writing if the two differ in any byte or count, if a run does not have the plan or
the statuses its case claims, or if the small budget did not cut the launch chunks the case says it cuts.
tests/test_points_calls_gpu.py demands these bits, counts and plans of every later library and capi.py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import points_calls_cases as PC  # noqa: E402


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "points_calls_parent.npz")
    for k in ("MEDGP_WGRAD_DEEP", "MEDGP_LA_PARK", "MEDGP_V0", "MEDGP_NO_CLASSES", "MEDGP_DEBUG_FAIL_ATTEMPTS", "MEDGP_MULTI_CU", "MEDGP_CHOLINV_NW",
              "MEDGP_POSTERIOR_BUDGET_GB"):
        os.environ.pop(k, None)
    out, labels, bad, seen = {}, None, [], {}
    for fam, budget, name in PC.RUNS:
        (arrs, counts, plan, res), (arrs2, counts2, plan2, _) = PC.run(fam, budget, name), PC.run(fam, budget, name)
        if labels is None:
            labels = sorted(counts)
        key = f"{fam}/{budget}/{name}/"
        same = counts == counts2 and plan == plan2 and len(arrs) == len(arrs2) and all(
            a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(arrs, arrs2))
        if not same:
            bad.append(key + " not run-to-run stable")
        if plan != PC.PLAN["A" if fam == "none" else fam]:
            bad.append(key + f" plan {plan}")
        st = np.asarray(PC.statuses(name, res)).tolist()
        want = [0] * len(st)
        if name.split("/")[0] in ("mean_nlml_grad", "basis_nlml_grad") and not (fam == "S" and name.startswith("mean")):
            want[PC.FAILED] = -1
        if st != want:
            bad.append(key + f" status {st}")
        seen[(fam, budget, name)] = counts
        if budget == "small":
            lab, nd, ns = PC.chunk_label(name), seen[(fam, "default", name)][PC.chunk_label(name)], counts[PC.chunk_label(name)]
            if PC.cut_possible(fam, name):
                if not ns > nd:
                    bad.append(key + f" {lab}: {ns} launches under the small budget, {nd} at the default: no chunk was cut")
                # chunks that are runs of tiles: at the default one launch per class that has points (a class without launches nothing)
                if lab != "k_pvjp_cot" and "joint" not in name and not ns > nd == PC.CLASSES_WITH_POINTS[fam]:
                    bad.append(key + f" {lab}: {ns} launches, {nd} at the default, for {PC.CLASSES_WITH_POINTS[fam]} classes with points")
            if name.startswith("posterior_vjp"):      # one more chunk: the cut between the two entries of the class of two
                ncot = PC.NCOT if name.endswith("custom") else 1
                if ns != nd + (ncot if PC.cut_possible(fam, name) else 0):
                    bad.append(key + f" {lab}: {ns} launches, {nd} at the default")
        out[key + "counts"] = np.array([counts[k] for k in labels], dtype=np.int64)
        out[key + "plan"] = np.array(plan, dtype=np.int64).reshape(-1, 2)
        out[key + "n"] = np.array(len(arrs), dtype=np.int64)
        for i, a in enumerate(arrs):
            out[key + str(i)] = np.ascontiguousarray(a)
        print(key, "status", st, "launches", sum(counts.values()), PC.chunk_label(name), counts[PC.chunk_label(name)], "arrays", len(arrs),
              "stable" if same else "UNSTABLE", flush=True)
    if bad:
        sys.exit("nothing written:\n" + "\n".join(bad))
    out["labels"] = np.array(labels)
    np.savez_compressed(dst, **out)
    size = os.path.getsize(dst)
    print("wrote", dst, size, "bytes")
    if size >= 1 << 20:
        os.remove(dst)
        sys.exit("the fixture would pass 1 MiB: nothing kept")


if __name__ == "__main__":
    main()
