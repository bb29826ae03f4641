"""Price medgp_functional_batch against the route a caller had before, and measure what that route loses on change scores.

  python scratch/functional_pricing.py time [--patients 64] [--reps 5]
      64 patients x N = 512, D = 24, Q = 5, R = 8; per patient 24 means over 24 h windows, 25 Gauss-Legendre nodes each (600 nodes).
      medgp_functional_batch against medgp_posterior_joint_batch (cov only) on the 600 nodes + the host's a^T (C - diag sigma^2) a.
      Kernel times come from medgp_profile_read (HIP events around every launch), wall is the whole Python call; the two calls
      alternate in one process, the fastest and the slowest of --reps calls after a warm-up call are printed.
  python scratch/functional_pricing.py accuracy
      The 0.25 h change scores of the parity cases of tests/functional_cases.py: fvar from the fp32 C of the joint call (two nodes per
      score, the noise peeled off the diagonal, the quadratic form in fp64) and from medgp_functional_batch, both against
      tests/functional_ref.py, in fp32 ulps of max(|ref|, 1e-3 S) (the bar of the GPU tests is 2) and relative to |ref| itself."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import medgp_amd  # noqa: E402
from medgp_amd import functionals as FN, synth  # noqa: E402


def price(a):
    P, N, D, Q, R, W, NODES = a.patients, 512, 24, 5, 8, 24, 25
    pts, th = synth.cohort(2024, P, D, N, Q=Q, R=R)
    ctx = medgp_amd.Context(7, Q, D, R)
    ctx.reserve(P, N, P)
    ctx.set_patients(np.arange(P), pts)
    slots = np.arange(P)
    lists = []
    for p, (m, t, y) in enumerate(pts):
        t0s = np.linspace(float(t.min()), float(t.max()) - 24.0, W)
        lists.append([FN.window_mean(w % D, float(t0), float(t0) + 24.0, NODES) for w, t0 in enumerate(t0s)])
    packed = [FN.pack(fs) for fs in lists]
    m2s, t2s, ws = [pk[1] for pk in packed], [pk[2] for pk in packed], [pk[3] for pk in packed]
    sig2 = [np.exp(2.0 * th[p, :D])[m2s[p]] for p in range(P)]
    print(f"{P} patients x N = {N}, D = {D}, Q = {Q}, R = {R}; {W} window means of {NODES} nodes per patient ({W * NODES} nodes); "
          f"route(s) after the first call below", flush=True)

    def functional():
        return ctx.functionals(slots, th, packed)

    def joint():
        out, st, cst = ctx.posterior_joint(slots, th, m2s, t2s, eps_list=None, cov=True)
        res = []
        for p in range(P):
            mean, var, Cm, _ = out[p]
            Cl = Cm.astype(np.float64) - np.diag(sig2[p])
            fm, fv = np.empty(W), np.empty(W)
            for w in range(W):
                s = slice(w * NODES, (w + 1) * NODES)
                fm[w] = ws[p][s] @ mean[s].astype(np.float64)
                fv[w] = ws[p][s] @ Cl[s, s] @ ws[p][s]
            res.append((fm, fv))
        return res

    fo, _ = functional()
    jo = joint()
    print("plan:", ctx.last_plan())
    dm = max(float(np.abs(fo[p][0] - jo[p][0]).max()) for p in range(P))
    dv = max(float(np.abs(fo[p][1] - jo[p][1]).max() / np.abs(fo[p][1]).max()) for p in range(P))
    print(f"the two routes agree: max |fmean - a^T mean| = {dm:.3g}, max |fvar - a^T C a| / max fvar = {dv:.3g}")
    ctx.profile_enable(True)
    rows = {"functional": [], "joint": []}
    for _ in range(a.reps):
        for name, fn in (("functional", functional), ("joint", joint)):
            ctx.profile_reset()
            t0 = time.perf_counter()
            fn()
            wall = time.perf_counter() - t0
            pr = ctx.profile_read()
            rows[name].append((wall, pr))
    ctx.profile_enable(False)
    inference = ("k_posterior", "k_postcov", "k_prep")
    for name in rows:
        walls = [r[0] * 1e3 for r in rows[name]]
        allk = [sum(v[0] for v in r[1].values()) for r in rows[name]]
        line = f"{name}: wall {min(walls):.2f} - {max(walls):.2f} ms; all kernels {min(allk):.3f} - {max(allk):.3f} ms"
        for k in inference:
            ms = [r[1][k][0] for r in rows[name]]
            line += f"; {k} {min(ms):.3f} - {max(ms):.3f} ms ({rows[name][0][1][k][1]} launches)"
        print(line, flush=True)
    ctx.close()


def accuracy(a):
    import functional_cases as FC
    import posterior_ref as PR
    print("fvar of the 0.25 h change scores (kind 3 of functional_cases.mix), error in fp32 ulps of max(|ref|, 1e-3 S) and relative to |ref|")
    for name in ("parity_d3", "parity_d24", "q17", "se", "sm"):
        fam, pts, th, qs = FC.case_data(name)
        kidx, Q, D, R = fam
        ctx = medgp_amd.Context(kidx, Q, D, R)
        ctx.reserve(len(pts), max(p[1].shape[0] for p in pts), len(pts))
        for s, (m, t, y) in enumerate(pts):
            ctx.set_patient(s, m if kidx == 7 else None, t, y)
        slots = np.arange(len(pts))
        out, st = ctx.functionals(slots, th, FC.call_list(qs))
        sel, m2s, t2s = [], [], []
        for p in range(len(pts)):
            toff, m2, t2, w = qs[p]
            idx = np.arange(3, len(toff) - 1, FC.KINDS)
            terms = np.concatenate([np.arange(toff[f], toff[f + 1]) for f in idx])
            sel.append(idx)
            m2s.append(m2[terms])
            t2s.append(t2[terms])
        jout, jst, _ = ctx.posterior_joint(slots, th, m2s if kidx == 7 else None, t2s, eps_list=None, cov=True)
        ctx.close()
        worst = {"fp32 C": [0.0, 0.0], "functional": [0.0, 0.0]}
        for p in range(len(pts)):
            ref = np.asarray(FC.case_ref(name, p)[1], np.float64)
            S = np.abs(ref).max()
            r = ref[sel[p]]
            Cl = jout[p][2].astype(np.float64) - np.diag(PR.noise_var(kidx, D, th[p], m2s[p] if kidx == 7 else np.zeros(len(t2s[p]), np.int32)))
            aw = np.array([1.0, -1.0])
            viaC = np.array([aw @ Cl[2 * k:2 * k + 2, 2 * k:2 * k + 2] @ aw for k in range(len(r))])
            for key, v in (("fp32 C", viaC), ("functional", out[p][1][sel[p]].astype(np.float64))):
                e = np.abs(v - r)
                worst[key][0] = max(worst[key][0], float((e / (2.0 ** -23 * np.maximum(np.abs(r), 1e-3 * S))).max()))
                worst[key][1] = max(worst[key][1], float((e / np.abs(r)).max()))
        print(f"{name}: " + "; ".join(f"{k}: {v[0]:.3g} ulps, {v[1]:.3g} relative" for k, v in worst.items()), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["time", "accuracy"])
    ap.add_argument("--patients", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    (price if args.what == "time" else accuracy)(args)
