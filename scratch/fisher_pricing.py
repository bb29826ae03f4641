"""Price one direction of medgp_fisher_vec next to one medgp_nlml_grad gradient call on the same batch, same build, one session.

  python scratch/fisher_pricing.py            512 patients x N = 512, D = 24, Q = 5, R = 8, route pinned

Kernel times come from medgp_profile_read (HIP events around every launch), best of --reps calls after a warm-up call.  The cost of
ONE direction is the difference between a call with nvec = 2 and a call with nvec = 1 (both share the one factorisation and the
one k_loo_kinv); the kernels of its own are listed as well.
MFMA flop per patient with n' = n rounded up to 64 (fp64 MFMA peak 78.6 TFLOP/s):
  k_cholinv        factor + inverse                                            ~ n'^3 / 3 + n'^3 / 3 ... (not counted here)
  k_wgrad          W tile = U_I U_J^T, columns >= 64 I, lower tiles             ~ n'^3 / 3
  k_loo_kinv       the same product, stored                                     ~ n'^3 / 3
  k_fisher_t       T = P Kdot, all tiles, all columns                           2 n'^3
  k_fisher_wgrad   G = T P^T, lower tiles, all columns                          ~ n'^3
Phase 3 (the pair loop, identical in k_wgrad and k_fisher_wgrad) and k_fisher_kdot's pair loop are not MFMA work."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import medgp_amd  # noqa: E402
from medgp_amd import synth  # noqa: E402

PEAK = 78.6e12
KERNELS = ("k_prep", "k_assemble", "k_cholinv", "k_la_step", "k_la_aux", "k_wgrad", "k_loo_kinv", "k_fisher_prep", "k_fisher_kdot", "k_fisher_t",
           "k_fisher_wgrad", "k_epilogue")


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

    def rate(name, fl, ms):
        print(f"    {name}: {fl:.3e} MFMA flop in {ms:.3f} ms (whole kernel) -> {fl / (ms * 1e-3) / 1e12:.2f} TFLOP/s = {100 * fl / (ms * 1e-3) / PEAK:.1f} % of fp64 peak")

    T = (N + 63) // 64
    npad = 64 * T
    tri_fl = P * sum(2.0 * 64 * 64 * (npad - 64 * i) * (i + 1) for i in range(T))
    low_fl = P * 2.0 * 64 * 64 * npad * T * (T + 1) / 2
    all_fl = P * 2.0 * npad ** 3
    wall_n, pr_n = timed(lambda: ctx.nlml_grad(slots, th, True))
    print(f"medgp_nlml_grad(grad): wall {wall_n * 1e3:.2f} ms, kernels {total(pr_n):.3f} ms; {line(pr_n)}")
    wall_1, pr_1 = timed(lambda: ctx.fisher_vec(slots, th, V[:, :1]))
    print(f"medgp_fisher_vec(nvec = 1): wall {wall_1 * 1e3:.2f} ms, kernels {total(pr_1):.3f} ms; {line(pr_1)}")
    wall_2, pr_2 = timed(lambda: ctx.fisher_vec(slots, th, V))
    print(f"medgp_fisher_vec(nvec = 2): wall {wall_2 * 1e3:.2f} ms, kernels {total(pr_2):.3f} ms; {line(pr_2)}")
    one = total(pr_2) - total(pr_1)
    own = sum(pr_1[k][0] for k in ("k_fisher_prep", "k_fisher_kdot", "k_fisher_t", "k_fisher_wgrad", "k_epilogue"))
    print(f"one direction: {one:.3f} ms of kernels (nvec 2 - nvec 1; its own kernels in the nvec = 1 call: {own:.3f} ms) = "
          f"{one / total(pr_n):.2f} x the kernels of one medgp_nlml_grad gradient call ({total(pr_n):.3f} ms)")
    rate("k_wgrad (medgp_nlml_grad)", tri_fl, pr_n["k_wgrad"][0])
    rate("k_loo_kinv", tri_fl, pr_1["k_loo_kinv"][0])
    rate("k_fisher_t", all_fl, pr_1["k_fisher_t"][0])
    rate("k_fisher_wgrad", low_fl, pr_1["k_fisher_wgrad"][0])
    ctx.close()


if __name__ == "__main__":
    main()
