"""Price medgp_mean_nlml_grad in both modes, and medgp_mean_posterior_batch, at the headline shape next to one medgp_nlml_grad of the
same build.

  python scratch/mean_pricing.py            512 patients x N = 512, D = 24, Q = 5, R = 8, 24 points per patient, route pinned

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
from medgp_amd import baseline, synth  # noqa: E402

KERNELS = ("k_prep", "k_assemble", "k_cholinv", "k_la_step", "k_la_aux", "k_wgrad", "k_epilogue", "k_pjvp_solve", "k_posterior", "k_mean_g", "k_mean_small",
           "k_mean_panel", "k_mean_wgrad", "k_mean_post")


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
    g = np.random.Generator(np.random.Philox(key=[2024, 10]))
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

    wall_g, pg = timed(lambda: ctx.nlml_grad(slots, th, True))
    print(f"medgp_nlml_grad: wall {wall_g * 1e3:.2f} ms, kernels {total(pg):.3f} ms; {line(pg)}")
    wall_m, pm = timed(lambda: ctx.mean_nlml_grad(slots, th, b0, lam))
    print(f"medgp_mean_nlml_grad(MARGINAL): wall {wall_m * 1e3:.2f} ms, kernels {total(pm):.3f} ms; {line(pm)}")
    wall_f, pf = timed(lambda: ctx.mean_nlml_grad(slots, th, b0, fixed=True))
    print(f"medgp_mean_nlml_grad(FIXED): wall {wall_f * 1e3:.2f} ms, kernels {total(pf):.3f} ms; {line(pf)}")
    wall_p, pp = timed(lambda: ctx.posterior(slots, th, m2, t2, parts=False))
    print(f"medgp_posterior_batch: wall {wall_p * 1e3:.2f} ms, kernels {total(pp):.3f} ms; {line(pp)}")
    wall_q, pq = timed(lambda: ctx.mean_posterior(slots, th, m2, t2, b0, lam))
    print(f"medgp_mean_posterior_batch(MARGINAL): wall {wall_q * 1e3:.2f} ms, kernels {total(pq):.3f} ms; {line(pq)}")
    print(f"MARGINAL = {total(pm) / total(pg):.2f} x, FIXED = {total(pf) / total(pg):.2f} x medgp_nlml_grad; k_mean_wgrad / k_wgrad = "
          f"{pm['k_mean_wgrad'][0] / pg['k_wgrad'][0]:.2f} (MARGINAL), {pf['k_mean_wgrad'][0] / pg['k_wgrad'][0]:.2f} (FIXED); "
          f"mean posterior = {total(pq) / total(pp):.2f} x medgp_posterior_batch")
    ctx.close()


if __name__ == "__main__":
    main()
