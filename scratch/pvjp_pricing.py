"""Price medgp_posterior_vjp_batch (built-in NLPD) at the headline shape next to (a) one medgp_nlml_grad and (b) the forward-mode
route to the same gradient: H directions of medgp_posterior_jvp_batch, priced as the cost of one more direction times H.

  python scratch/pvjp_pricing.py            512 patients x N = 512, D = 24, Q = 5, R = 8, 24 points per patient, route pinned

Kernel times come from medgp_profile_read (HIP events around every launch): a warm-up call, then --reps calls, the median call by its
kernel total."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import medgp_amd  # noqa: E402
from medgp_amd import synth  # noqa: E402

KERNELS = ("k_prep", "k_assemble", "k_cholinv", "k_la_step", "k_la_aux", "k_wgrad", "k_epilogue", "k_pjvp_solve", "k_fisher_prep", "k_fisher_kdot",
           "k_pjvp_u", "k_pjvp_dir", "k_pvjp_cot", "k_pvjp_wgrad", "k_pvjp_cross", "k_pvjp_finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=24)
    a = ap.parse_args()
    P, N, D, Q, R = 512, 512, 24, 5, 8
    pts, th = synth.cohort(2024, P, D, N, Q=Q, R=R)
    H = th.shape[1]
    ctx = medgp_amd.Context(7, Q, D, R)
    ctx.reserve(P, N, P)
    ctx.set_patients(np.arange(P), pts)
    ctx.pin_route(True)
    slots = np.arange(P)
    g = np.random.Generator(np.random.Philox(key=[2024, 9]))
    V = g.standard_normal((P, 2, H))
    t2 = [g.uniform(float(t.min()) - 24.0, float(t.max()) + 24.0, a.points).astype(np.float32) for _, t, _ in pts]
    m2 = [g.integers(0, D, a.points).astype(np.int32) for _ in pts]
    y2 = [g.standard_normal(a.points) for _ in pts]
    print(f"{P} patients x N = {N}, D = {D}, Q = {Q}, R = {R}, H = {H}, {a.points} points per patient, route pinned", flush=True)

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

    wall_g, pg = timed(lambda: ctx.nlml_grad(slots, th, True))
    print(f"medgp_nlml_grad: wall {wall_g * 1e3:.2f} ms, kernels {total(pg):.3f} ms; {line(pg)}")
    wall_v, pv = timed(lambda: ctx.posterior_vjp(slots, th, m2, t2, loss="nlpd", y2_list=y2, want_posterior=False))
    print(f"medgp_posterior_vjp_batch(NLPD): wall {wall_v * 1e3:.2f} ms, kernels {total(pv):.3f} ms; {line(pv)}")
    p2 = timed(lambda: ctx.posterior_jvp(slots, th, m2, t2, V, want_posterior=False))[1]
    p1 = timed(lambda: ctx.posterior_jvp(slots, th, m2, t2, V[:, :1], want_posterior=False))[1]
    per = total(p2) - total(p1)
    print(f"medgp_posterior_jvp_batch: nvec = 2 {total(p2):.3f} ms, nvec = 1 {total(p1):.3f} ms of kernels; one more direction {per:.3f} ms")
    print(f"the new call = {total(pv) / total(pg):.2f} x medgp_nlml_grad; the JVP route to the same gradient, H = {H} directions: {per * H:.0f} ms "
          f"of kernels, {per * H / total(pv):.0f} x the new call")
    print(f"k_pvjp_wgrad / k_wgrad = {pv['k_pvjp_wgrad'][0] / pg['k_wgrad'][0]:.2f}")
    ctx.close()


if __name__ == "__main__":
    main()
