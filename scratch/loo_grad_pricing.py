"""Price medgp_loo_grad next to medgp_nlml_grad (objective + gradient) on the same build.

  python scratch/loo_grad_pricing.py headline     512 patients x N = 512, D = 24, Q = 5, R = 8
  python scratch/loo_grad_pricing.py big          one patient, N = 2048, D = 24, Q = 5, R = 8

Kernel times come from medgp_profile_read (HIP events around every launch), best of --reps calls after a warm-up call.
Flop counts (fp64 MFMA peak 78.6 TFLOP/s), per patient with n' = n rounded up to 64 and T = n' / 64:
  k_wgrad      phase 1, W tile (I, J) = U_I U_J^T over the columns >= 64 I: 2 * 64 * 64 * (n' - 64 I) per lower tile  ~ n'^3 / 3
  k_loo_kinv   the same product, stored as the full symmetric P                                                       ~ n'^3 / 3
  k_loo_wgrad  phase 1, G tile = P_I diag(s) P_J^T over all n' columns: 2 * 64 * 64 * n' per lower tile                ~ n'^3
  k_loo_vec    d from U (n^2 / 2 elements), v = P u (n^2 elements): bandwidth, 8 bytes per element
Phase 3 (the pair loop, identical in k_wgrad and k_loo_wgrad) is not MFMA work and is left out of the counts."""
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
HBM = 8.0e12
KERNELS = ("k_prep", "k_assemble", "k_cholinv", "k_la_step", "k_la_aux", "k_wgrad", "k_loo_kinv", "k_loo_vec", "k_loo_wgrad", "k_epilogue")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["headline", "big"])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    P, N, D, Q, R = (512, 512, 24, 5, 8) if a.case == "headline" else (1, 2048, 24, 5, 8)
    pts, th = synth.cohort(2024, P, D, N, Q=Q, R=R)
    ctx = medgp_amd.Context(7, Q, D, R)
    ctx.reserve(P, N, P)
    ctx.set_patients(np.arange(P), pts)
    slots = np.arange(P)
    print(f"case {a.case}: {P} patients x N = {N}, D = {D}, Q = {Q}", flush=True)

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
        return min(res, key=lambda r: r[0])

    def line(pr):
        return "; ".join(f"{k} {pr[k][0]:.3f} ms ({pr[k][1]})" for k in KERNELS if pr[k][1])

    def total(pr):
        return sum(pr[k][0] for k in KERNELS)

    T = (N + 63) // 64
    npad = 64 * T
    tri_fl = P * sum(2.0 * 64 * 64 * (npad - 64 * i) * (i + 1) for i in range(T))   # U U^T on the lower tiles, k >= 64 I
    full_fl = P * 2.0 * 64 * 64 * npad * T * (T + 1) / 2                             # P diag(s) P on the lower tiles, all k
    wall_n, pr_n = timed(lambda: ctx.nlml_grad(slots, th, True))
    print(f"medgp_nlml_grad(grad): wall {wall_n * 1e3:.2f} ms, kernels {total(pr_n):.3f} ms; {line(pr_n)}; route(s) {ctx.last_plan()}")
    wall_0, pr_0 = timed(lambda: ctx.loo_grad(slots, th, False))
    print(f"medgp_loo_grad(flag_grad = 0): wall {wall_0 * 1e3:.2f} ms, kernels {total(pr_0):.3f} ms; {line(pr_0)}")
    wall_l, pr_l = timed(lambda: ctx.loo_grad(slots, th, True))
    print(f"medgp_loo_grad(flag_grad = 1): wall {wall_l * 1e3:.2f} ms, kernels {total(pr_l):.3f} ms ({total(pr_l) / total(pr_n):.2f} x the kernels of "
          f"medgp_nlml_grad, wall {wall_l / wall_n:.2f} x); {line(pr_l)}")
    for name, pr, k, fl in (("medgp_nlml_grad", pr_n, "k_wgrad", tri_fl), ("medgp_loo_grad", pr_l, "k_loo_kinv", tri_fl), ("medgp_loo_grad", pr_l, "k_loo_wgrad", full_fl)):
        ms = pr[k][0]
        print(f"    {k} ({name}): {fl:.3e} MFMA flop in {ms:.3f} ms (whole kernel) -> {fl / (ms * 1e-3) / 1e12:.2f} TFLOP/s = {100 * fl / (ms * 1e-3) / PEAK:.1f} % of fp64 peak")
    byts = 8.0 * P * (N * N / 2 + N * N)
    ms = pr_l["k_loo_vec"][0]
    print(f"    k_loo_vec (both passes): {byts:.3e} bytes in {ms:.3f} ms -> {byts / (ms * 1e-3) / 1e12:.2f} TB/s = {100 * byts / (ms * 1e-3) / HBM:.1f} % of HBM peak")
    print(f"    MFMA flop of the gradient path: medgp_loo_grad {tri_fl + full_fl:.3e}, medgp_nlml_grad {tri_fl:.3e} ({(tri_fl + full_fl) / tri_fl:.2f} x)")
    ctx.close()


if __name__ == "__main__":
    main()
