"""Price medgp_lgo_grad next to medgp_loo_grad and medgp_nlml_grad (objective + gradient) on the same build, in one session.

  python scratch/lgo_grad_pricing.py headline     512 patients x N = 512, D = 24, Q = 5, R = 8; groups by covariate and by 24-h window
  python scratch/lgo_grad_pricing.py big          one patient, N = 2048, D = 24, Q = 5, R = 8; groups by covariate

Kernel times come from medgp_profile_read (HIP events around every launch), best of --reps calls after a warm-up call.
Flop and byte counts (fp64 MFMA peak 78.6 TFLOP/s, HBM 8 TB/s), per patient with n' = n rounded up to 64, T = n' / 64, and per group
of m > 1 members with m' = m rounded up to 64, t = m' / 64:
  k_loo_kinv    P = U U^T on the lower tiles, columns >= 64 I:          2 * 64 * 64 * (n' - 64 I) per lower tile            ~ n'^3 / 3
  k_lgo_wgrad   phase 1, G tile = P_I Tt_J^T over all n' columns:       2 * 64 * 64 * n' per lower tile                     ~ n'^3
  k_loo_gram    M tile (I, J) from the gathered rows of U:              at most 2 * 64 * 64 * n' per lower tile pair of the group
  k_lgo_inv     column tile c of X = R^-1, block rows k > c:            2 * 64 * 64 * 64 (k - c) per (c, k)                 ~ m'^3 / 3
                (+ one 64 x 64 substitution per (c, k), not MFMA work and not counted)
  k_lgo_s       S tile (I, J) = X^T X from block row I on:              2 * 64 * 64 * (m' - 64 I) per lower tile pair       ~ m'^3 / 3
  k_lgo_t       Tt[:, B] = P[:, B] S:                                   2 * n' * m' * m' per group
  k_lgo_vec     k_lgo_prep reads P and writes Tt: 16 n'^2 bytes per patient (the mask and the sum of J are negligible)
Phase 3 (the pair loop, identical in k_wgrad, k_loo_wgrad and k_lgo_wgrad) is not MFMA work and is left out of the counts."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import medgp_amd  # noqa: E402
from medgp_amd import crossval, synth  # noqa: E402

PEAK = 78.6e12
HBM = 8.0e12
KERNELS = ("k_prep", "k_assemble", "k_cholinv", "k_la_step", "k_la_aux", "k_wgrad", "k_loo_kinv", "k_loo_vec", "k_loo_wgrad", "k_loo_gram",
           "k_postfactor", "k_loo_solve", "k_lgo_vec", "k_lgo_inv", "k_lgo_s", "k_lgo_t", "k_lgo_wgrad", "k_epilogue")


def group_flops(npad, sizes):
    """MFMA flop of (k_lgo_inv, k_lgo_s, k_lgo_t) for one patient whose larger groups have the given sizes"""
    inv = s = t = 0.0
    for m in sizes:
        if m < 2:
            continue
        nt = (m + 63) // 64
        mpad = 64 * nt
        inv += sum(2.0 * 64 * 64 * 64 * (k - c) for c in range(nt) for k in range(c + 1, nt))
        s += sum(2.0 * 64 * 64 * (mpad - 64 * i) * (i + 1) for i in range(nt))
        t += 2.0 * npad * mpad * mpad
    return inv, s, t


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

    def rate(name, fl, ms):
        print(f"    {name}: {fl:.3e} MFMA flop in {ms:.3f} ms (whole kernel) -> {fl / (ms * 1e-3) / 1e12:.2f} TFLOP/s = {100 * fl / (ms * 1e-3) / PEAK:.1f} % of fp64 peak")

    T = (N + 63) // 64
    npad = 64 * T
    tri_fl = P * sum(2.0 * 64 * 64 * (npad - 64 * i) * (i + 1) for i in range(T))
    full_fl = P * 2.0 * 64 * 64 * npad * T * (T + 1) / 2
    wall_n, pr_n = timed(lambda: ctx.nlml_grad(slots, th, True))
    print(f"medgp_nlml_grad(grad): wall {wall_n * 1e3:.2f} ms, kernels {total(pr_n):.3f} ms; {line(pr_n)}; route(s) {ctx.last_plan()}")
    wall_l, pr_l = timed(lambda: ctx.loo_grad(slots, th, True))
    print(f"medgp_loo_grad(flag_grad = 1): wall {wall_l * 1e3:.2f} ms, kernels {total(pr_l):.3f} ms; {line(pr_l)}")
    schemes = [("by covariate", [crossval.by_covariate(m, D)[0] for m, t, y in pts])]
    if a.case == "headline":
        schemes.append(("24-h windows", [crossval.by_window(t, 24.0)[0] for m, t, y in pts]))
    for name, gs in schemes:
        sizes = [np.bincount(g[g >= 0]) for g in gs]
        allm = np.concatenate(sizes)
        print(f"groups {name}: {int((allm > 0).sum())} non-empty groups in the call, {int((allm == 1).sum())} singletons, sizes up to {int(allm.max())}, mean {allm[allm > 0].mean():.1f}")
        wall_0, pr_0 = timed(lambda: ctx.lgo_grad(slots, th, gs, False))
        print(f"  medgp_lgo_grad(flag_grad = 0): wall {wall_0 * 1e3:.2f} ms, kernels {total(pr_0):.3f} ms; {line(pr_0)}")
        wall_g, pr_g = timed(lambda: ctx.lgo_grad(slots, th, gs, True))
        print(f"  medgp_lgo_grad(flag_grad = 1): wall {wall_g * 1e3:.2f} ms, kernels {total(pr_g):.3f} ms ({total(pr_g) / total(pr_l):.2f} x the kernels of "
              f"medgp_loo_grad, {total(pr_g) / total(pr_n):.2f} x medgp_nlml_grad; wall {wall_g / wall_l:.2f} x, {wall_g / wall_n:.2f} x); {line(pr_g)}")
        fl = np.sum([group_flops(npad, s) for s in sizes], axis=0)
        rate("k_loo_kinv", tri_fl, pr_g["k_loo_kinv"][0])
        rate("k_lgo_wgrad", full_fl, pr_g["k_lgo_wgrad"][0])
        for k, f in zip(("k_lgo_inv", "k_lgo_s", "k_lgo_t"), fl):
            if pr_g[k][1] and f > 0:
                rate(k, f, pr_g[k][0])
        byts = 16.0 * P * npad * npad
        ms = pr_g["k_lgo_vec"][0]
        print(f"    k_lgo_vec (mask, prep, J): {byts:.3e} bytes in {ms:.3f} ms -> {byts / (ms * 1e-3) / 1e12:.2f} TB/s = {100 * byts / (ms * 1e-3) / HBM:.1f} % of HBM peak")
    rate("k_wgrad (medgp_nlml_grad)", tri_fl, pr_n["k_wgrad"][0])
    rate("k_loo_wgrad (medgp_loo_grad)", full_fl, pr_l["k_loo_wgrad"][0])
    ctx.close()


if __name__ == "__main__":
    main()
