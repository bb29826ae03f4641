"""Price one direction of medgp_hess_vec next to one direction of medgp_fisher_vec and one medgp_nlml_grad gradient call on the same
batch, same build, one session; and the once-per-call moment pass next to k_wgrad.

  python scratch/hess_pricing.py            512 patients x N = 512, D = 24, Q = 5, R = 8, route pinned

Kernel times come from medgp_profile_read (HIP events around every launch), best of --reps calls after a warm-up call.  The cost of
ONE direction is the difference between a call with nvec = 2 and a call with nvec = 1 (both share the one factorisation, the one
k_loo_kinv and the one W pass); the kernels of its own are listed as well."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import medgp_amd  # noqa: E402
from medgp_amd import synth  # noqa: E402

KERNELS = ("k_prep", "k_assemble", "k_cholinv", "k_la_step", "k_la_aux", "k_wgrad", "k_loo_kinv", "k_hess_moments", "k_hess_slabsum",
           "k_fisher_prep", "k_fisher_kdot", "k_fisher_t", "k_fisher_wgrad", "k_hess_beta", "k_hess_wgrad", "k_hess_epilogue", "k_epilogue")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    P, N, D, Q, R = 512, 512, 24, 5, 8
    pts, th = synth.cohort(2024, P, D, N, Q=Q, R=R)
    ctx = medgp_amd.Context(7, Q, D, R)
    ctx.reserve(P, N, P)
    ctx.set_patients(np.arange(P), pts)
    ctx.pin_route(True)
    slots = np.arange(P)
    V = np.random.Generator(np.random.Philox(key=[2024, 7])).standard_normal((P, 2, th.shape[1]))
    print(f"{P} patients x N = {N}, D = {D}, Q = {Q}, R = {R}, route pinned", flush=True)

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
        return min(res, key=lambda r: sum(r[1][k][0] for k in KERNELS))

    def line(pr):
        return "; ".join(f"{k} {pr[k][0]:.3f} ms ({pr[k][1]})" for k in KERNELS if pr[k][1])

    def total(pr):
        return sum(pr[k][0] for k in KERNELS)

    wall_n, pr_n = timed(lambda: ctx.nlml_grad(slots, th, True))
    print(f"medgp_nlml_grad(grad): wall {wall_n * 1e3:.2f} ms, kernels {total(pr_n):.3f} ms; {line(pr_n)}")
    f1 = timed(lambda: ctx.fisher_vec(slots, th, V[:, :1]))[1]
    f2 = timed(lambda: ctx.fisher_vec(slots, th, V))[1]
    print(f"medgp_fisher_vec(nvec = 1): kernels {total(f1):.3f} ms; {line(f1)}")
    print(f"medgp_fisher_vec(nvec = 2): kernels {total(f2):.3f} ms; {line(f2)}")
    wall_1, h1 = timed(lambda: ctx.hess_vec(slots, th, V[:, :1]))
    wall_2, h2 = timed(lambda: ctx.hess_vec(slots, th, V))
    print(f"medgp_hess_vec(nvec = 1): wall {wall_1 * 1e3:.2f} ms, kernels {total(h1):.3f} ms; {line(h1)}")
    print(f"medgp_hess_vec(nvec = 2): wall {wall_2 * 1e3:.2f} ms, kernels {total(h2):.3f} ms; {line(h2)}")
    hg = timed(lambda: ctx.hess_vec(slots, th, V[:, :1], want_grad=True))[1]
    print(f"medgp_hess_vec(nvec = 1, grad): kernels {total(hg):.3f} ms; k_epilogue {hg['k_epilogue'][0]:.3f} ms ({hg['k_epilogue'][1]})")
    one_h, one_f = total(h2) - total(h1), total(f2) - total(f1)
    print(f"one Hessian direction: {one_h:.3f} ms of kernels (nvec 2 - nvec 1) = {one_h / one_f:.2f} x one Fisher direction ({one_f:.3f} ms) = "
          f"{one_h / total(pr_n):.2f} x the kernels of one medgp_nlml_grad gradient call ({total(pr_n):.3f} ms)")
    once = h1["k_hess_moments"][0] + h1["k_hess_slabsum"][0]
    print(f"once per call: k_hess_moments {h1['k_hess_moments'][0]:.3f} ms + k_hess_slabsum {h1['k_hess_slabsum'][0]:.3f} ms = {once:.3f} ms "
          f"= {h1['k_hess_moments'][0] / pr_n['k_wgrad'][0]:.2f} x k_wgrad ({pr_n['k_wgrad'][0]:.3f} ms)")
    ctx.close()


if __name__ == "__main__":
    main()
