"""Price medgp_posterior_batch against the same points through medgp_fit_predict (k_predict, one workgroup per point).

  python scratch/posterior_pricing.py headline [--kp-patients 32]   512 patients x N = 512, D = 24, Q = 5, R = 8;
                                                                    64 grid times x 24 covariates = 1536 points per patient
  python scratch/posterior_pricing.py big                           one patient, D = 64, N = 4096 (look-ahead route), 6400 points

Kernel times come from medgp_profile_read (HIP events around every launch).  (b) runs medgp_fit_predict once per patient
for --kp-patients patients and scales k_predict linearly to the cohort (its work is per point and independent across
patients).  The flop count of the posterior solve is n^2 * m (forward substitution of m right-hand sides, 2 flop per
multiply-add, half the matrix); the fraction is against 78.6 TFLOP/s fp64 MFMA peak."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import medgp_amd  # noqa: E402
from medgp_amd import synth  # noqa: E402

PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["headline", "big"])
    ap.add_argument("--kp-patients", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-kpredict", action="store_true")
    a = ap.parse_args()
    if a.case == "headline":
        P, N, D, Q, R, G = 512, 512, 24, 5, 8, 64
    else:
        P, N, D, Q, R, G = 1, 4096, 64, 5, 8, 100
    pts, th = synth.cohort(2024, P, D, N, Q=Q, R=R)
    ctx = medgp_amd.Context(7, Q, D, R)
    ctx.reserve(P, N, P)
    ctx.set_patients(np.arange(P), pts)
    m2s, t2s = [], []
    for m, t, y in pts:
        tg = np.linspace(float(t.min()), float(t.max()), G).astype(np.float32)
        m2s.append(np.repeat(np.arange(D, dtype=np.int32), G))
        t2s.append(np.tile(tg, D))
    M = sum(x.shape[0] for x in t2s)
    out, st = ctx.posterior(np.arange(P), th, m2s, t2s)   # warm-up (allocations, code objects)
    assert np.all(st == 0), st
    print(f"case {a.case}: {P} patients x N = {N}, D = {D}, Q = {Q}; {M} points ({M // P} per patient); route(s) {ctx.last_plan()}")
    ctx.profile_enable(True)
    res = []
    for _ in range(a.reps):
        ctx.profile_reset()
        t0 = time.perf_counter()
        ctx.posterior(np.arange(P), th, m2s, t2s)
        wall = time.perf_counter() - t0
        pr = ctx.profile_read()
        res.append((wall, pr))
    wall, pr = min(res, key=lambda r: r[1]["k_posterior"][0])
    fit_ms = sum(pr[k][0] for k in ("k_prep", "k_assemble", "k_cholinv", "k_la_step", "k_la_aux"))
    ka, kp = pr["k_alpha"], pr["k_posterior"]
    flop = float(N) * N * M
    print(f"(a) medgp_posterior_batch: wall {wall * 1e3:.1f} ms; factorisation kernels {fit_ms:.2f} ms; "
          f"k_alpha {ka[0]:.3f} ms ({ka[1]} launches); k_posterior {kp[0]:.3f} ms ({kp[1]} launches)")
    print(f"    k_posterior: n^2 m = {flop:.3e} flop -> {flop / (kp[0] * 1e-3) / 1e12:.2f} TFLOP/s = {100 * flop / (kp[0] * 1e-3) / PEAK:.1f} % of fp64 peak")
    if a.no_kpredict:
        return
    kpp = min(a.kp_patients, P)
    ctx.profile_reset()
    t0 = time.perf_counter()
    for p in range(kpp):
        mean, var, s = ctx.fit_predict(p, th[p], m2s[p], t2s[p])
        assert s == 0
    wall_b = time.perf_counter() - t0
    pr = ctx.profile_read()
    kpred = pr["k_predict"][0] * P / kpp
    print(f"(b) medgp_fit_predict x {kpp} patients: wall {wall_b * 1e3:.1f} ms; k_predict {pr['k_predict'][0]:.2f} ms measured "
          f"-> {kpred:.1f} ms for {P} patients")
    post = ka[0] + kp[0]
    print(f"    ratio (k_alpha + k_posterior) / k_predict = {post / kpred:.4f}  (k_predict / posterior = {kpred / post:.1f} x)")
    # outputs of (a) and (b) agree
    mean_b, var_b, _ = ctx.fit_predict(0, th[0], m2s[0], t2s[0])
    print(f"    patient 0: max |mean a - b| / max|mean| = {np.abs(out[0][0] - mean_b).max() / np.abs(mean_b).max():.2e}, "
          f"max |var a - b| / max|var| = {np.abs(out[0][1] - var_b).max() / np.abs(var_b).max():.2e}")
    ctx.close()


if __name__ == "__main__":
    main()
