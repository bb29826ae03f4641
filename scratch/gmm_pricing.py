#!/usr/bin/env python3
"""Price of the kernel-clustering step at the reference's defaults (not a pass criterion): the 73-dimensional features of
the spectral components of a synthetic 4096-patient LMC-SM cohort (Q = 5: 20 480 points), K = 1 .. 5, 10 restarts each, max_iter 2000,
tol 1e-3 -- ONE medgp_gmm_fit call of 50 runs.  Reports the whole call (wall and the HIP-event time from the first to the last launch),
the numpy definition (tests/gmm_ref.py) on the first start of every K, and scikit-learn from the same starts if it is installed.  The
split by kernel comes from running this script with --device-only under `rocprofv3 --kernel-trace --stats`.
Writes profiles/gmm_pricing.txt.

    python scratch/gmm_pricing.py [--patients 4096] [--cpu-iters 20] [--device-only]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from medgp_amd import capi, clustering  # noqa: E402
import gmm_cases as GC  # noqa: E402
import gmm_ref as GR  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patients", type=int, default=4096)
    ap.add_argument("--cpu-iters", type=int, default=20, help="iterations of the CPU legs (they are priced per iteration)")
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    Q, D, R, init_num, max_iter, tol = 5, 2, 2, 10, 2000, 1e-3
    rng = np.random.default_rng(4096)
    hyp = GC.synthetic_hypers(rng, a.patients, Q, D, R)
    _, _, feat = clustering.extract_kernel_feature("LMC-SM", Q, D, R, np.arange(a.patients), hyp)
    ks = np.array([K for K in range(1, Q + 1) for _ in range(init_num)], dtype=np.int32)
    l0 = np.stack([clustering.init_labels(feat, int(K), rng) for K in ks])
    lines = [f"gmm pricing: {feat.shape[0]} x {feat.shape[1]} component features of {a.patients} synthetic patients, K = 1 .. {Q}, "
             f"{init_num} restarts, max_iter {max_iter}, tol {tol}: one call of {len(ks)} runs"]
    capi.gmm_fit(feat[:256], ks[:1], l0[:1, :256], max_iter=1)     # first-call costs (module load) stay out of the timing
    t0 = time.perf_counter()
    lb, bic, nit, st, _, _, _, _, ms = capi.gmm_fit(feat, ks, l0, max_iter=max_iter, tol=tol, full=True)
    wall = time.perf_counter() - t0
    best, per_k = clustering.select_model(ks, lb, bic, st)
    lines.append(f"device: wall {wall * 1e3:.1f} ms, first to last launch {ms:.1f} ms; iterations per run min {nit.min()} median "
                 f"{int(np.median(nit))} max {nit.max()} (the call runs max = {nit.max()} rounds of 7 launches: {ms / max(nit.max(), 1):.3f} ms per round); "
                 f"status counts converged {int(np.sum(st == 1))} max_iter {int(np.sum(st == 0))} failed {int(np.sum(st < 0))}; selected K = {ks[best]}")
    lines.append("device: BIC per K " + ", ".join(f"{K}: {b:.1f}" for K, b in per_k))
    if not a.device_only:
        for K in range(1, Q + 1):
            r = int(np.flatnonzero(ks == K)[0])
            t0 = time.perf_counter()
            o = GR.gmm_fit_one(feat, K, l0[r], a.cpu_iters, 0.0)
            t = time.perf_counter() - t0
            line = f"numpy definition K = {K}: {t / max(o['n_iter'], 1) * 1e3:.1f} ms per iteration ({o['n_iter']} iterations)"
            try:
                t0 = time.perf_counter()
                s = GR.sklearn_fit(feat, K, l0[r], a.cpu_iters, 0.0)
                line += f"; scikit-learn {(time.perf_counter() - t0) / max(s['n_iter'], 1) * 1e3:.1f} ms per iteration"
            except ImportError:
                line += "; scikit-learn not installed"
            lines.append(line)
        lines.append(f"CPU threads: {os.environ.get('OMP_NUM_THREADS', 'default')}; the device call advances all {len(ks)} runs per round, a CPU "
                     "run advances one")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(ROOT, "profiles", "gmm_pricing.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
