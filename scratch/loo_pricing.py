"""Price medgp_loo_batch on the two shapes of scratch/posterior_joint_pricing.py.

  python scratch/loo_pricing.py headline [--alt-patients 8]   512 patients x N = 512, D = 24, Q = 5, R = 8: singletons, by covariate
  python scratch/loo_pricing.py big [--alt-patients 1]        one patient, D = 64, N = 4096: by covariate (64 groups of 64)

Kernel times come from medgp_profile_read (HIP events around every launch), best of --reps calls after a warm-up call, next
to the MEDGP_FLAG_KEEP_FACTOR nlml call that forms the same factor, U = L^-T and alpha on the same build.
Counts used for the fractions (fp64 MFMA peak 78.6 TFLOP/s, HBM 8 TB/s):
  k_loo_diag   reads the upper triangle of U once: 8 n^2 / 2 bytes per patient; 2 flop per element (bandwidth bound)
  k_loo_gram   M_B = U_B U_B^T: for the lower tile pairs of a group 2 * 64 * 64 * (n - first row of tile I) flop per pair; counted
               here algorithmically as sum over groups of m^2 (n - mean first row) ~ m^2 n / 2 for groups spread over the rows
  k_postfactor m^3 / 3 per group, k_loo_solve m^3 / 3 (the triangular inverse) + 2 m^2 (the vector solves) per group
The alternative a caller has today: medgp_get_factor per entry (alpha and L^-1 as floats) + loo_ref.via_inverse on the host's
cores, measured on --alt-patients patients and scaled to the cohort."""
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
KERNELS = ("k_prep", "k_assemble", "k_cholinv", "k_la_step", "k_la_aux", "k_loo_diag", "k_loo_gram", "k_postfactor", "k_loo_solve")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["headline", "big"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--alt-patients", type=int, default=8)
    ap.add_argument("--no-alt", action="store_true")
    a = ap.parse_args()
    if a.case == "headline":
        P, N, D, Q, R = 512, 512, 24, 5, 8
        schemes = (("singletons", None), ("by covariate", "covariate"))
    else:
        P, N, D, Q, R = 1, 4096, 64, 5, 8
        schemes = (("by covariate", "covariate"),)
    pts, th = synth.cohort(2024, P, D, N, Q=Q, R=R)
    ctx = medgp_amd.Context(7, Q, D, R)
    ctx.reserve(P, N, P)
    ctx.set_patients(np.arange(P), pts)
    slots = np.arange(P)
    print(f"case {a.case}: {P} patients x N = {N}, D = {D}, Q = {Q}; MEDGP_POSTERIOR_BUDGET_GB = "
          f"{os.environ.get('MEDGP_POSTERIOR_BUDGET_GB', '2 (default)')}", flush=True)

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

    wall_k, pr_k = timed(lambda: ctx.nlml_grad(slots, th, False, keep_factor=True))
    print(f"medgp_nlml_grad(KEEP_FACTOR): wall {wall_k * 1e3:.1f} ms; {line(pr_k)}; route(s) {ctx.last_plan()}", flush=True)
    for name, groups in schemes:
        wall, pr = timed(lambda: ctx.loo(slots, th, groups))
        print(f"medgp_loo_batch, {name}: wall {wall * 1e3:.1f} ms ({wall / wall_k:.2f} x the KEEP_FACTOR call); {line(pr)}")
        if groups is None:
            byts = 8.0 * N * N / 2 * P
            ms = pr["k_loo_diag"][0]
            print(f"    k_loo_diag: {byts:.3e} bytes -> {byts / (ms * 1e-3) / 1e12:.2f} TB/s = {100 * byts / (ms * 1e-3) / HBM:.1f} % of HBM peak")
        else:
            sizes = [np.bincount(p[0], minlength=D) for p in pts]
            gram = sum(float(m) * m * N / 2 for s in sizes for m in s if m > 1)
            fac = sum(float(m) ** 3 / 3 for s in sizes for m in s if m > 1)
            for k, fl in (("k_loo_gram", gram), ("k_postfactor", fac), ("k_loo_solve", fac)):
                ms = pr[k][0]
                print(f"    {k}: {fl:.3e} flop -> {fl / (ms * 1e-3) / 1e12:.3f} TFLOP/s = {100 * fl / (ms * 1e-3) / PEAK:.2f} % of fp64 peak")
        sys.stdout.flush()
    if a.no_alt:
        return
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import loo_ref  # noqa: E402
    ap_ = min(a.alt_patients, P)
    ctx.nlml_grad(slots, th, False, keep_factor=True)
    t0 = time.perf_counter()
    for p in range(ap_):
        ctx.get_factor(p, N)
    wall_f = (time.perf_counter() - t0) * P / ap_
    for name, groups in schemes:
        t0 = time.perf_counter()
        for p in range(ap_):
            g = None if groups is None else pts[p][0]
            loo_ref.via_inverse(7, Q, D, R, *pts[p], th[p], g, None if g is None else D)
        wall_n = (time.perf_counter() - t0) * P / ap_
        print(f"alternative, {name}: medgp_get_factor per entry {wall_f * 1e3:.0f} ms + numpy via_inverse {wall_n * 1e3:.0f} ms for {P} patients "
              f"(measured on {ap_}, OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS')})")
    ctx.close()


if __name__ == "__main__":
    main()
