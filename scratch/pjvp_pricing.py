"""Price medgp_posterior_jvp_batch at the headline shape next to the finite-difference route it replaces: 2 nvec calls of
medgp_posterior_batch (two per direction).

  python scratch/pjvp_pricing.py            512 patients x N = 512, D = 24, Q = 5, R = 8, 24 points per patient, nvec = 4, route pinned

Kernel times come from medgp_profile_read (HIP events around every launch): a warm-up call, then --reps calls, the median call by its
kernel total.  The cost of ONE direction is also taken as the difference between a call with nvec = 4 and a call with nvec = 3."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import medgp_amd  # noqa: E402
from medgp_amd import synth  # noqa: E402

KERNELS = ("k_prep", "k_assemble", "k_cholinv", "k_la_step", "k_la_aux", "k_posterior", "k_pjvp_solve", "k_fisher_prep", "k_fisher_kdot",
           "k_pjvp_u", "k_pjvp_dir")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=24)
    ap.add_argument("--nvec", type=int, default=4)
    a = ap.parse_args()
    P, N, D, Q, R = 512, 512, 24, 5, 8
    pts, th = synth.cohort(2024, P, D, N, Q=Q, R=R)
    ctx = medgp_amd.Context(7, Q, D, R)
    ctx.reserve(P, N, P)
    ctx.set_patients(np.arange(P), pts)
    ctx.pin_route(True)
    slots = np.arange(P)
    g = np.random.Generator(np.random.Philox(key=[2024, 8]))
    V = g.standard_normal((P, a.nvec, th.shape[1]))
    t2 = [g.uniform(float(t.min()) - 24.0, float(t.max()) + 24.0, a.points).astype(np.float32) for _, t, _ in pts]
    m2 = [g.integers(0, D, a.points).astype(np.int32) for _ in pts]
    print(f"{P} patients x N = {N}, D = {D}, Q = {Q}, R = {R}, {a.points} points per patient, nvec = {a.nvec}, route pinned", flush=True)

    def total(pr):
        return sum(pr[k][0] for k in KERNELS)

    def timed(fn):
        fn()   # warm-up (allocations, code objects)
        ctx.profile_enable(True)
        res = []
        for _ in range(a.reps):
            ctx.profile_reset()
            t0 = time.perf_counter()
            fn()
            res.append((time.perf_counter() - t0, ctx.profile_read()))
        ctx.profile_enable(False)
        res.sort(key=lambda r: total(r[1]))
        return res[len(res) // 2]

    def line(pr):
        return "; ".join(f"{k} {pr[k][0]:.3f} ms ({pr[k][1]})" for k in KERNELS if pr[k][1])

    wall_p, pp = timed(lambda: ctx.posterior(slots, th, m2, t2, parts=False))
    print(f"medgp_posterior_batch: wall {wall_p * 1e3:.2f} ms, kernels {total(pp):.3f} ms; {line(pp)}")
    wall_j, pj = timed(lambda: ctx.posterior_jvp(slots, th, m2, t2, V))
    print(f"medgp_posterior_jvp_batch(nvec = {a.nvec}): wall {wall_j * 1e3:.2f} ms, kernels {total(pj):.3f} ms; {line(pj)}")
    if a.nvec > 1:
        pk = timed(lambda: ctx.posterior_jvp(slots, th, m2, t2, V[:, :-1]))[1]
        print(f"medgp_posterior_jvp_batch(nvec = {a.nvec - 1}): kernels {total(pk):.3f} ms; one more direction {total(pj) - total(pk):.3f} ms")
    fd = 2 * a.nvec * total(pp)
    print(f"the differencing route, {2 * a.nvec} posterior calls: {fd:.3f} ms of kernels; the new call {total(pj):.3f} ms = {total(pj) / fd:.2f} x")
    ctx.close()


if __name__ == "__main__":
    main()
