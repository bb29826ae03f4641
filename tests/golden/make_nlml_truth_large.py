"""Writes tests/golden/nlml_truth_large.npz: the long-double truth and the errors of the three legitimate fp64 programs for the
patients of nlml_truth.large_cases() that are too slow to recompute in every test run (n > nlml_truth.FIXTURE_ABOVE_N), plus the
one cheap patient the CPU test recomputes to check the stored bits (nlml_truth.FIXTURE_BIT_CHECK).

Run by hand from the repository root after `make -C oracle` (program (a) is the oracle), never by the suite:

    python tests/golden/make_nlml_truth_large.py [--jobs J] [--parts DIR]

Uses the project's own code only (tests/nlml_truth.py, oracle/).  One process per patient, J at a time (the long-double code is
single-threaded numpy; n = 2048 takes about two minutes, n = 2880 six, n = 4096 at D = 64 twenty-five, and 1 to 5 GB each).  With
--parts every finished patient is kept as DIR/<case>_<p>.npz and a part whose input hash still matches is reused, so an interrupted
run resumes.  Prints time, errors, budgets and spreads per patient; exits non-zero when a patient misses a condition of
tests/test_nlml_truth.py (status 0, both budgets under their caps, both spreads within M / 4): then choose another draw in
nlml_truth.DRAWS by the rule written there.

Stored per patient i: ids[i] = "<case id>:<patient>", sha256[i] of the input bytes (nlml_truth.input_sha256), status[i] (the
oracle's), nlml_hi[i] + nlml_lo[i] and grad_hi_<i> + grad_lo_<i> (two float64 whose sum in long double is the truth exactly),
en[i, 3], eg[i, 3] (errors of the oracle, of the float64 run, of the float64 run in the device's form).
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


def _part_path(parts, cid, p):
    return os.path.join(parts, f"{cid}_{p}.npz") if parts else None


def _one(arg):
    cid, p, parts = arg
    case = [c for c in T.large_cases() if c["id"] == cid][0]
    sha = T.input_sha256(case, p)
    path = _part_path(parts, cid, p)
    if path and os.path.exists(path):
        with np.load(path) as z:
            if str(z["sha256"]) == sha:
                print(f"{cid}:{p}: reusing {path}", flush=True)
                return {k: z[k] for k in z.files}
    t0 = time.time()
    r = T.compute_programs(case, p)
    if r["status"] < 0:
        raise SystemExit(f"{cid}:{p}: oracle status {r['status']}")
    nh, nl = T.split_hi_lo(r["truth"][0])
    gh, gl = T.split_hi_lo(r["truth"][1])
    out = dict(sha256=np.array(sha), status=np.int64(r["status"]), nlml_hi=nh, nlml_lo=nl, grad_hi=gh, grad_lo=gl,
               en=np.array(r["en"]), eg=np.array(r["eg"]), secs=np.float64(time.time() - t0))
    if path:
        np.savez(path, **out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--parts", default=None)
    a = ap.parse_args()
    if a.parts:
        os.makedirs(a.parts, exist_ok=True)
    todo = [(c["id"], p, a.parts) for c, p in T.fixture_patients()]
    with multiprocessing.Pool(a.jobs) as pool:
        res = pool.map(_one, todo, chunksize=1)
    bad = 0
    for (cid, p, _), r in zip(todo, res):
        en, eg = list(r["en"]), list(r["eg"])
        bn, bg = T.budget(en, T.M_NLML), T.budget(eg, T.M_GRAD)
        sn, sg = T.spread(en), T.spread(eg)
        ok = int(r["status"]) == 0 and bn < T.NLML_BUDGET_CAP and bg < T.GRAD_BUDGET_CAP and sn <= T.M_NLML / 4 and sg <= T.M_GRAD / 4
        bad += not ok
        print(f"{cid}:{p} H={r['grad_hi'].shape[0]} {float(r['secs']):.0f} s status {int(r['status'])} "
              f"E_nlml {en[0]:.2e} {en[1]:.2e} {en[2]:.2e} E_grad {eg[0]:.2e} {eg[1]:.2e} {eg[2]:.2e} "
              f"budget {bn:.2e} / {bg:.2e} spread {sn:.1f} / {sg:.1f} {'ok' if ok else 'MISSES A CONDITION'}")
    out = dict(ids=np.array([f"{cid}:{p}" for cid, p, _ in todo]), sha256=np.array([str(r["sha256"]) for r in res]),
               status=np.array([int(r["status"]) for r in res], np.int64),
               nlml_hi=np.array([float(r["nlml_hi"]) for r in res]), nlml_lo=np.array([float(r["nlml_lo"]) for r in res]),
               en=np.array([r["en"] for r in res]), eg=np.array([r["eg"] for r in res]))
    for i, r in enumerate(res):
        out[f"grad_hi_{i}"], out[f"grad_lo_{i}"] = r["grad_hi"], r["grad_lo"]
    np.savez_compressed(T.LARGE_FIXTURE, **out)
    print(f"wrote {T.LARGE_FIXTURE}: {os.path.getsize(T.LARGE_FIXTURE)} bytes, {len(res)} patients")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
