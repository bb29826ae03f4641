"""Price medgp_functional_joint_batch against the route a caller had before for the covariance BETWEEN functionals.

  python scratch/functional_joint_pricing.py [--patients 64] [--reps 5]
      64 patients x N = 512, D = 24, Q = 5, R = 8; per patient 24 means over 24 h windows, 25 Gauss-Legendre nodes each (600 nodes).
      medgp_functional_joint_batch (24 x 24 floats per patient) against medgp_posterior_joint_batch (cov only) on the 600 nodes
      (600 x 600 floats per patient) + the host's A^T (C - diag sigma^2) A.  Kernel times come from medgp_profile_read (HIP events
      around every launch), wall is the whole Python call; the two calls alternate in one process, the fastest and the slowest of
      --reps calls after a warm-up call are printed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
    A = []
    for p in range(P):
        Ap = np.zeros((W * NODES, W))
        for w in range(W):
            Ap[w * NODES:(w + 1) * NODES, w] = ws[p][w * NODES:(w + 1) * NODES]
        A.append(Ap)
    print(f"{P} patients x N = {N}, D = {D}, Q = {Q}, R = {R}; {W} window means of {NODES} nodes per patient ({W * NODES} nodes)", flush=True)

    def functional_joint():
        out, _ = ctx.functionals_joint(slots, th, packed)
        return [o[2] for o in out]

    def joint():
        out, st, cst = ctx.posterior_joint(slots, th, m2s, t2s, eps_list=None, cov=True)
        return [A[p].T @ (out[p][2].astype(np.float64) - np.diag(sig2[p])) @ A[p] for p in range(P)]

    fo = functional_joint()
    jo = joint()
    print("plan:", ctx.last_plan())
    d = max(float(np.abs(fo[p] - jo[p]).max() / np.abs(fo[p]).max()) for p in range(P))
    print(f"the two routes agree: max |fcov - A^T C A| / max |fcov| = {d:.3g}")
    ctx.profile_enable(True)
    rows = {"functional_joint": [], "joint": []}
    for _ in range(a.reps):
        for name, fn in (("functional_joint", functional_joint), ("joint", joint)):
            ctx.profile_reset()
            t0 = time.perf_counter()
            fn()
            wall = time.perf_counter() - t0
            rows[name].append((wall, ctx.profile_read()))
    ctx.profile_enable(False)
    for name in rows:
        walls = [r[0] * 1e3 for r in rows[name]]
        allk = [sum(v[0] for v in r[1].values()) for r in rows[name]]
        line = f"{name}: wall {min(walls):.2f} - {max(walls):.2f} ms; all kernels {min(allk):.3f} - {max(allk):.3f} ms"
        for k in ("k_posterior", "k_postcov", "k_prep"):
            ms = [r[1][k][0] for r in rows[name]]
            line += f"; {k} {min(ms):.3f} - {max(ms):.3f} ms ({rows[name][0][1][k][1]} launches)"
        print(line, flush=True)
    ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--patients", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    price(ap.parse_args())
