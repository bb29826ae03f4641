"""Price medgp_forecast_batch: rolling-origin forecasts of every observation of a cohort at horizons {0, 6, 24} h.

  python scratch/forecast_pricing.py [--sample 512] [--reps 3]

512 patients x N = 512, D = 24, Q = 5, R = 8, each sorted by time (covariates interleaved: the caller-order copy);
medgp_amd.forecast.rolling_origin gives 3 x 512 = 1536 points per patient.  Three figures, kernel times from medgp_profile_read
(HIP events around every launch), best of --reps calls after a warm-up:
  (a) k_forecast on those points with their prefixes,
  (b) k_posterior on the same points conditioning on everything (medgp_posterior_batch without the decomposition): the
      ceiling the panel cut-off should beat,
  (c) the route a caller had before: one slot per (patient, prefix), medgp_fit_predict_batch -- run on a SAMPLE of --sample
      points with prefix >= 3 (each uploads its own history and pays its own factorisation) and EXTRAPOLATED linearly to all
      points (the sample is uniform over the points, so its mean cost per point is the cohort's).
The flop count of the forecast solve is sum_j p_j^2 (forward substitution of column j stopped at row p_j, 2 flop per
multiply-add, half the matrix) rounded up to whole 64-row panels and whole tiles by the kernel."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import medgp_amd  # noqa: E402
from medgp_amd import forecast, synth  # noqa: E402

PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sample", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    P, N, D, Q, R = 512, 512, 24, 5, 8
    hs = [0.0, 6.0, 24.0]
    pts, th = synth.cohort(2024, P, D, N, Q=Q, R=R)
    pts = [tuple(x[np.argsort(p[1], kind="stable")] for x in p) for p in pts]   # time order
    ctx = medgp_amd.Context(7, Q, D, R)
    ctx.reserve(P, N, P)
    ctx.set_patients(np.arange(P), pts)
    ro = [forecast.rolling_origin(m, t, y, hs) for m, t, y in pts]
    m2s, t2s, y2s, pfs = ([r[k] for r in ro] for k in range(4))
    M = sum(x.shape[0] for x in t2s)
    allpf = np.concatenate(pfs).astype(np.float64)
    out, st = ctx.forecast(np.arange(P), th, m2s, t2s, pfs, y2s)   # warm-up (allocations, code objects)
    assert np.all(st == 0), st
    print(f"{P} patients x N = {N}, D = {D}, Q = {Q}, time-ordered; horizons {hs} h; {M} points ({M // P} per patient); "
          f"mean prefix {allpf.mean():.1f}, prefix 0: {int((allpf == 0).sum())} points; route(s) {ctx.last_plan()}")
    ctx.profile_enable(True)

    def best(call, key):
        res = []
        for _ in range(a.reps):
            ctx.profile_reset()
            t0 = time.perf_counter()
            call()
            res.append((time.perf_counter() - t0, ctx.profile_read()))
        return min(res, key=lambda r: r[1][key][0])

    fit = lambda pr: sum(pr[k][0] for k in ("k_prep", "k_assemble", "k_cholinv", "k_la_step", "k_la_aux"))
    wall, pr = best(lambda: ctx.forecast(np.arange(P), th, m2s, t2s, pfs, y2s), "k_forecast")
    kf = pr["k_forecast"]
    fit_a = fit(pr)
    flop = float((allpf ** 2).sum())
    print(f"(a) medgp_forecast_batch: wall {wall * 1e3:.1f} ms; factorisation kernels {fit(pr):.2f} ms; k_forecast {kf[0]:.3f} ms ({kf[1]} launches)")
    print(f"    k_forecast: sum p^2 = {flop:.3e} flop -> {flop / (kf[0] * 1e-3) / 1e12:.2f} TFLOP/s = {100 * flop / (kf[0] * 1e-3) / PEAK:.1f} % of fp64 peak")
    wall, pr = best(lambda: ctx.posterior(np.arange(P), th, m2s, t2s, parts=False), "k_posterior")
    kp = pr["k_posterior"]
    print(f"(b) medgp_posterior_batch (same points, all data, no decomposition): wall {wall * 1e3:.1f} ms; factorisation kernels {fit(pr):.2f} ms; "
          f"k_posterior {kp[0]:.3f} ms ({kp[1]} launches)")
    print(f"    k_forecast / k_posterior = {kf[0] / kp[0]:.3f}  (sum p^2 / (n^2 m) = {flop / (float(N) * N * M):.3f})")
    ctx.close()
    # (c) one slot per sampled (patient, prefix)
    g = np.random.default_rng(7)
    owner = np.repeat(np.arange(P), [x.shape[0] for x in t2s])
    local = np.concatenate([np.arange(x.shape[0]) for x in t2s])
    cand = np.flatnonzero(allpf >= 3)
    S = min(a.sample, cand.shape[0])
    pick = g.choice(cand, size=S, replace=False)
    c2 = medgp_amd.Context(7, Q, D, R)
    c2.reserve(S, N, S)
    hist = []
    for j in pick:
        b, k = owner[j], local[j]
        p = int(pfs[b][k])
        hist.append(tuple(x[:p] for x in pts[b]))
    c2.set_patients(np.arange(S), hist)
    th2 = th[owner[pick]]
    m2 = np.array([m2s[owner[j]][local[j]] for j in pick], np.int32)
    t2 = np.array([t2s[owner[j]][local[j]] for j in pick], np.float32)
    mean, var, st2 = c2.fit_predict_batch(np.arange(S), th2, m2, t2)   # warm-up
    assert np.all(st2 == 0), st2
    dev = np.array([out[owner[j]][0][local[j]] for j in pick])
    c2.profile_enable(True)
    res = []
    for _ in range(a.reps):
        c2.profile_reset()
        t0 = time.perf_counter()
        c2.fit_predict_batch(np.arange(S), th2, m2, t2)
        res.append((time.perf_counter() - t0, c2.profile_read()))
    wall, pr = min(res, key=lambda r: sum(v[0] for v in r[1].values()))
    ks = sum(v[0] for v in pr.values())
    print(f"(c) medgp_fit_predict_batch, one slot per (patient, prefix): SAMPLE of {S} of the {cand.shape[0]} points with prefix >= 3 "
          f"(mean prefix {np.mean([h[1].shape[0] for h in hist]):.1f}): wall {wall * 1e3:.1f} ms, kernels {ks:.3f} ms")
    ext = ks * cand.shape[0] / S
    print(f"    EXTRAPOLATED to all {cand.shape[0]} such points: kernels {ext:.0f} ms, against {fit_a + kf[0]:.2f} ms (factorisation + k_forecast) "
          f"of (a): {ext / (fit_a + kf[0]):.0f} x")
    print(f"    sample: max |mean (a) - (c)| / max|mean| = {np.abs(dev - mean).max() / np.abs(mean).max():.2e}")
    c2.close()


if __name__ == "__main__":
    main()
