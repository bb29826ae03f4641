"""Writes tests/golden/objective_truth_large.npz: the long-double truth and the errors of the two legitimate fp64 programs for every
entry of objective_large.entries() -- medgp_loo_grad, medgp_lgo_grad, medgp_forecast_grad and medgp_fisher_vec on the patients of the
large sweep, N = 513 .. 2048 (and the D = 64 patient).

Run by hand from the repository root, never by the suite:

    python tests/golden/make_objective_truth_large.py [--jobs J] [--parts DIR] [--only SUBSTRING]

Uses the project's own code only (tests/objective_large.py and the truth modules it names).  One process per entry, J at a time, the
slowest first (single-threaded long-double numpy: seconds up to n = 640, 10 to 60 s at n = 1024, minutes at n = 2048; under 2 GB
each).  With --parts every finished entry is kept as DIR/<key>.npz and a part whose input hash still matches is reused, so an
interrupted run resumes and a changed draw recomputes its own entries alone.  Prints time, cond(K), errors and budgets per entry and
exits non-zero when an entry misses a condition of tests/test_objective_large.py (both budgets under their caps, cond(K) <= COND_MAX):
then take the next draw in objective_large.DRAWS by the rule written there.  An optional n = 2048 entry that takes more than 30
minutes goes into objective_large.LONG_ABSENT.

Stored per entry i: keys[i] = "<case id>:<patient>:<objective>:<table>", sha256[i] of the input bytes (objective_large.input_sha256),
obj_hi[i] + obj_lo[i] and grad_hi_<i> + grad_lo_<i> (two float64 whose sum in long double is the truth exactly; grad is [nvec, H] and
obj 0 for the Fisher call), en[i, 2], eg[i, 2] (errors of the float64 run of the truth code and of the numpy.linalg program; en 0 for
the Fisher call), cond[i], secs[i].
"""
import argparse
import multiprocessing
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import nlml_truth as T  # noqa: E402
import objective_large as OL  # noqa: E402


def _one(arg):
    e, parts = arg
    key = OL.key_of(e)
    sha = OL.input_sha256(e)
    path = os.path.join(parts, key.replace(":", "_") + ".npz") if parts else None
    if path and os.path.exists(path):
        with np.load(path) as z:
            if str(z["sha256"]) == sha:
                print(f"{key}: reusing {path}", flush=True)
                return {k: z[k] for k in z.files}
    t0 = time.time()
    truth = OL.run_program(e, "truth")
    eb = OL.errors_of(e, OL.run_program(e, "b"), truth)
    ec = OL.errors_of(e, OL.run_program(e, "c"), truth)
    fisher = e[3] == "fisher"
    oh, ol = (np.float64(0), np.float64(0)) if fisher else T.split_hi_lo(truth[0])
    gh, gl = T.split_hi_lo(truth[1])
    out = dict(sha256=np.array(sha), obj_hi=oh, obj_lo=ol, grad_hi=gh, grad_lo=gl,
               en=np.array([0.0, 0.0] if fisher else [eb[0], ec[0]]), eg=np.array([eb[1], ec[1]]),
               cond=np.float64(OL.cond_of(*e[1:4])), secs=np.float64(time.time() - t0))
    if path:
        np.savez(path, **out)
    print(f"{key}: {float(out['secs']):.0f} s", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--parts", default=None)
    ap.add_argument("--only", default=None, help="compute the entries whose key contains this alone and write no fixture")
    a = ap.parse_args()
    if a.parts:
        os.makedirs(a.parts, exist_ok=True)
    todo = [e for e in OL.entries() if a.only is None or a.only in OL.key_of(e)]
    cost = {"loo": 1.0, "lgo": 2.0, "fc": 3.0, "fisher": 4.0}
    order = sorted(range(len(todo)), key=lambda i: -OL.n_of(todo[i][1], todo[i][2]) ** 3 * cost[todo[i][3]])
    with multiprocessing.Pool(a.jobs) as pool:
        got = pool.map(_one, [(todo[i], a.parts) for i in order], chunksize=1)
    res = [None] * len(todo)
    for i, r in zip(order, got):
        res[i] = r
    bad = 0
    for e, r in zip(todo, res):
        fisher = e[3] == "fisher"
        en, eg = list(r["en"]), list(r["eg"])
        bn = 0.0 if fisher else T.budget(en, OL.M_OBJ)
        bg = T.budget(eg, OL.M_FISHER if fisher else OL.M_GRAD)
        ok = bn <= OL.NLML_BUDGET_CAP and bg <= OL.GRAD_BUDGET_CAP and float(r["cond"]) <= OL.COND_MAX
        bad += not ok
        print(f"{OL.key_of(e)} n {OL.n_of(e[1], e[2])} H={r['grad_hi'].shape[-1]} {float(r['secs']):.0f} s cond {float(r['cond']):.3g} "
              f"E_obj {en[0]:.2e} {en[1]:.2e} E_grad {eg[0]:.2e} {eg[1]:.2e} budget {bn:.2e} / {bg:.2e} "
              f"{'ok' if ok else 'MISSES A CONDITION'}")
    if a.only is not None:
        sys.exit(1 if bad else 0)
    out = dict(keys=np.array([OL.key_of(e) for e in todo]), sha256=np.array([str(r["sha256"]) for r in res]),
               obj_hi=np.array([float(r["obj_hi"]) for r in res]), obj_lo=np.array([float(r["obj_lo"]) for r in res]),
               en=np.array([r["en"] for r in res]), eg=np.array([r["eg"] for r in res]),
               cond=np.array([float(r["cond"]) for r in res]), secs=np.array([float(r["secs"]) for r in res]))
    for i, r in enumerate(res):
        out[f"grad_hi_{i}"], out[f"grad_lo_{i}"] = r["grad_hi"], r["grad_lo"]
    np.savez_compressed(OL.FIXTURE, **out)
    print(f"wrote {OL.FIXTURE}: {os.path.getsize(OL.FIXTURE)} bytes, {len(res)} entries")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
