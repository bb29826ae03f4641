"""Price medgp_forecast_grad next to medgp_nlml_grad and medgp_loo_grad (objective + gradient) on the same build.

  python scratch/forecast_grad_pricing.py headline     512 patients x N = 512, D = 24, Q = 5, R = 8
  python scratch/forecast_grad_pricing.py big          one patient, N = 2048, D = 24, Q = 5, R = 8

Every patient is uploaded in time order (covariates interleaved: the factor is the caller-order one and the gradient body runs on
the grouped copy), horizons 0 h and 6 h (medgp_amd.forecast.training_prefix).  Kernel times come from medgp_profile_read (HIP events
around every launch), best of --reps calls after a warm-up call.  MFMA flop per patient, n' = n rounded up to 64, T = n' / 64
(fp64 MFMA peak 78.6 TFLOP/s):
  k_fc_t       tile (R, C), R <= C: 2 * 64 * 64 * (columns from max(64 R, pmin_C) to 64 (C + 1)): at most ~ n'^3 / 3 (full histories
               far back), less for a short horizon (the band is narrow); counted from the prefix table
  k_fc_wgrad   two products per lower tile over the scored column blocks: 2 * 2 * 64 * 64 * n' per tile                  ~ 2 n'^3
  k_wgrad      n'^3 / 3,  k_loo_kinv n'^3 / 3,  k_loo_wgrad n'^3   (scratch/loo_grad_pricing.py)
Phase 3 (the pair loop, identical in k_wgrad, k_loo_wgrad and k_fc_wgrad) is not MFMA work and is left out of the counts."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import medgp_amd  # noqa: E402
from medgp_amd import forecast, synth  # noqa: E402

PEAK = 78.6e12
KERNELS = ("k_prep", "k_assemble", "k_cholinv", "k_la_step", "k_la_aux", "k_wgrad", "k_loo_kinv", "k_loo_vec", "k_loo_wgrad",
           "k_fc_vec", "k_fc_t", "k_fc_scan", "k_fc_qm", "k_fc_tables", "k_fc_wgrad", "k_epilogue")


def t_flop(pf):
    n = pf.shape[0]
    T = (n + 63) // 64
    fl = 0.0
    for C in range(T):
        p = pf[64 * C:64 * C + 64]
        p = p[p >= 0]
        if p.size == 0:
            continue
        for R in range(C + 1):
            fl += 2.0 * 64 * 64 * (64 * (C + 1) - max(64 * R, int(p.min()) & ~31))
    return fl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["headline", "big"])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    P, N, D, Q, R = (512, 512, 24, 5, 8) if a.case == "headline" else (1, 2048, 24, 5, 8)
    pts, th = synth.cohort(2024, P, D, N, Q=Q, R=R)
    srt = []
    for m, t, y in pts:
        o = np.argsort(t, kind="stable")
        srt.append((m[o], t[o], y[o]))
    ctx = medgp_amd.Context(7, Q, D, R)
    ctx.reserve(P, N, P)
    ctx.set_patients(np.arange(P), srt)
    slots = np.arange(P)
    print(f"case {a.case}: {P} patients x N = {N}, D = {D}, Q = {Q}, uploaded in time order", flush=True)

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
    wall_n, pr_n = timed(lambda: ctx.nlml_grad(slots, th, True))
    print(f"medgp_nlml_grad(grad): wall {wall_n * 1e3:.2f} ms, kernels {total(pr_n):.3f} ms; {line(pr_n)}; route(s) {ctx.last_plan()}")
    wall_l, pr_l = timed(lambda: ctx.loo_grad(slots, th, True))
    print(f"medgp_loo_grad(flag_grad = 1): wall {wall_l * 1e3:.2f} ms, kernels {total(pr_l):.3f} ms; {line(pr_l)}")
    for h in (0.0, 6.0):
        pfs = [forecast.training_prefix(t, h) for _, t, _ in srt]
        wall_0, pr_0 = timed(lambda: ctx.forecast_grad(slots, th, pfs, 0))
        print(f"medgp_forecast_grad(horizon {h:g} h, flag_grad = 0): wall {wall_0 * 1e3:.2f} ms, kernels {total(pr_0):.3f} ms; {line(pr_0)}")
        wall_f, pr_f = timed(lambda: ctx.forecast_grad(slots, th, pfs, 1))
        print(f"medgp_forecast_grad(horizon {h:g} h, flag_grad = 1): wall {wall_f * 1e3:.2f} ms, kernels {total(pr_f):.3f} ms ({total(pr_f) / total(pr_n):.2f} x the "
              f"kernels of medgp_nlml_grad, {total(pr_f) / total(pr_l):.2f} x medgp_loo_grad; wall {wall_f / wall_n:.2f} x / {wall_f / wall_l:.2f} x); {line(pr_f)}")
        tfl = sum(t_flop(pf) for pf in pfs)
        wfl = P * 2 * 2.0 * 64 * 64 * npad * T * (T + 1) / 2
        for k, fl in (("k_fc_t", tfl), ("k_fc_wgrad", wfl)):
            ms = pr_f[k][0]
            print(f"    {k}: {fl:.3e} MFMA flop in {ms:.3f} ms (whole kernel) -> {fl / (ms * 1e-3) / 1e12:.2f} TFLOP/s = {100 * fl / (ms * 1e-3) / PEAK:.1f} % of fp64 peak")
    ctx.close()


if __name__ == "__main__":
    main()
