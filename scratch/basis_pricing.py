"""Price medgp_basis_nlml_grad and medgp_basis_posterior_batch at the headline shape: once with the indicator basis (p = 24) beside
medgp_mean_nlml_grad on the same data, once with a dense basis of p = 64 columns.

  python scratch/basis_pricing.py            512 patients x N = 512, D = 24, Q = 5, R = 8, 24 points per patient, route pinned

Kernel times come from medgp_profile_read (HIP events around every launch): a warm-up call, then --reps calls, the best call by its
kernel total."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import medgp_amd  # noqa: E402
from medgp_amd import baseline, basis, synth  # noqa: E402

KERNELS = ("k_prep", "k_assemble", "k_cholinv", "k_la_step", "k_la_aux", "k_wgrad", "k_epilogue", "k_pjvp_solve", "k_mean_g", "k_mean_small",
           "k_mean_panel", "k_mean_wgrad", "k_mean_post", "k_basis_g", "k_basis_small", "k_basis_post")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=24)
    a = ap.parse_args()
    P, N, D, Q, R = 512, 512, 24, 5, 8
    pts, th = synth.cohort(2024, P, D, N, Q=Q, R=R)
    ctx = medgp_amd.Context(7, Q, D, R)
    ctx.reserve(P, N, P)
    ctx.set_patients(np.arange(P), pts)
    ctx.pin_route(True)
    slots = np.arange(P)
    g = np.random.Generator(np.random.Philox(key=[2024, 11]))
    t2 = [g.uniform(float(t.min()) - 24.0, float(t.max()) + 24.0, a.points).astype(np.float32) for _, t, _ in pts]
    m2 = [g.integers(0, D, a.points).astype(np.int32) for _ in pts]
    b0, lam = baseline.standard_prior(D)
    print(f"{P} patients x N = {N}, D = {D}, Q = {Q}, R = {R}, H = {th.shape[1]}, {a.points} points per patient, route pinned; best of {a.reps}", flush=True)

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
        return min(res, key=lambda r: total(r[1]))

    def line(pr):
        return "; ".join(f"{k} {pr[k][0]:.3f} ms ({pr[k][1]})" for k in KERNELS if pr[k][1])

    wall, pm = timed(lambda: ctx.mean_nlml_grad(slots, th, b0, lam))
    print(f"medgp_mean_nlml_grad(MARGINAL): wall {wall * 1e3:.2f} ms, kernels {total(pm):.3f} ms; {line(pm)}")
    ind = basis.Design([basis.intercept(D)])
    t0 = time.perf_counter()
    ctx.set_basis(slots, [ind.design(m, t) for m, t, _ in pts])
    ctx.synchronize()
    print(f"medgp_set_basis(p = {D}): {1e3 * (time.perf_counter() - t0):.1f} ms wall with the host-side design matrices, {P * N * D * 8 / 1e6:.0f} MB")
    wall, pb = timed(lambda: ctx.basis_nlml_grad(slots, th, b0, lam))
    print(f"medgp_basis_nlml_grad(MARGINAL, indicator p = {D}): wall {wall * 1e3:.2f} ms, kernels {total(pb):.3f} ms; {line(pb)}")
    wall, pf = timed(lambda: ctx.basis_nlml_grad(slots, th, b0, fixed=True))
    print(f"medgp_basis_nlml_grad(FIXED, indicator p = {D}): wall {wall * 1e3:.2f} ms, kernels {total(pf):.3f} ms; {line(pf)}")
    h2 = [ind.design(m, t) for m, t in zip(m2, t2)]
    wall, pq = timed(lambda: ctx.basis_posterior(slots, th, m2, t2, h2, b0, lam))
    print(f"medgp_basis_posterior_batch(MARGINAL, indicator p = {D}): wall {wall * 1e3:.2f} ms, kernels {total(pq):.3f} ms; {line(pq)}")
    print(f"indicator basis = {total(pb) / total(pm):.2f} x medgp_mean_nlml_grad; k_basis_g / k_mean_panel = {pb['k_basis_g'][0] / pb['k_mean_panel'][0]:.2f}")
    p = 64
    H64 = [np.concatenate([np.ones((N, 1)), g.standard_normal((N, p - 1))], axis=1) for _ in pts]
    ctx.set_basis(slots, H64)
    b64, l64 = np.zeros(p), np.ones(p)
    wall, p64 = timed(lambda: ctx.basis_nlml_grad(slots, th, b64, l64))
    print(f"medgp_basis_nlml_grad(MARGINAL, dense p = {p}): wall {wall * 1e3:.2f} ms, kernels {total(p64):.3f} ms; {line(p64)}")
    h2 = [np.concatenate([np.ones((a.points, 1)), g.standard_normal((a.points, p - 1))], axis=1) for _ in pts]
    wall, q64 = timed(lambda: ctx.basis_posterior(slots, th, m2, t2, h2, b64, l64))
    print(f"medgp_basis_posterior_batch(MARGINAL, dense p = {p}): wall {wall * 1e3:.2f} ms, kernels {total(q64):.3f} ms; {line(q64)}")
    print(f"dense p = 64: {total(p64) / total(pm):.2f} x medgp_mean_nlml_grad; k_basis_g / k_mean_panel = {p64['k_basis_g'][0] / p64['k_mean_panel'][0]:.2f}")
    ctx.close()


if __name__ == "__main__":
    main()
