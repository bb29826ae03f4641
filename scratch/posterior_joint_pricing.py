"""Price medgp_posterior_joint_batch on the two shapes of scratch/posterior_pricing.py, nsamp = 16.

  python scratch/posterior_joint_pricing.py headline [--alt-patients 8]   512 patients x N = 512, D = 24, Q = 5, R = 8; 1536 points each
  python scratch/posterior_joint_pricing.py big [--alt-patients 1]        one patient, D = 64, N = 4096, 6400 points

Kernel times come from medgp_profile_read (HIP events around every launch), best of --reps calls after a warm-up call.
k_postcov's flop count is algorithmic: m^2 n for V^T V over the FULL m x m (2 flop per multiply-add, half the matrix) plus
m^2 / 2 pairs x Q components x ~30 flop for K**; the fraction is against 78.6 TFLOP/s fp64 MFMA peak.  The whole-call time is
put next to medgp_posterior_batch's for the same points (no decomposition).  The alternative a caller had before:
medgp_factor_batch (L and z to the host in fp64) + the numpy restatement (oracle Gram of training + test points, triangular
solve, V^T V, Cholesky, draw) on the host's cores, measured on --alt-patients patients and scaled to the cohort."""
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
PAIR_FLOP = 30.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["headline", "big"])
    ap.add_argument("--nsamp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--alt-patients", type=int, default=8)
    ap.add_argument("--no-alt", action="store_true")
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
    m = t2s[0].shape[0]
    M = m * P
    g = np.random.Generator(np.random.Philox(key=[2024, 1]))
    eps = [g.standard_normal((m, a.nsamp)) for _ in range(P)]
    slots = np.arange(P)
    print(f"case {a.case}: {P} patients x N = {N}, D = {D}, Q = {Q}; {m} points per patient, nsamp = {a.nsamp}; "
          f"MEDGP_POSTERIOR_BUDGET_GB = {os.environ.get('MEDGP_POSTERIOR_BUDGET_GB', '2 (default)')}", flush=True)

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

    wall_m, pr_m = timed(lambda: ctx.posterior(slots, th, m2s, t2s, parts=False))
    print(f"medgp_posterior_batch (marginals, no parts): wall {wall_m * 1e3:.1f} ms; k_posterior {pr_m['k_posterior'][0]:.3f} ms "
          f"({pr_m['k_posterior'][1]} launches); route(s) {ctx.last_plan()}", flush=True)
    flop = float(m) * m * N * P + 0.5 * m * m * Q * PAIR_FLOP * P
    for name, kw in (("samples only", dict(eps_list=eps, cov=False)), ("cov only", dict(eps_list=None, cov=True)),
                     ("cov + samples", dict(eps_list=eps, cov=True))):
        wall, pr = timed(lambda: ctx.posterior_joint(slots, th, m2s, t2s, **kw))
        kc, kf, kd, kp = pr["k_postcov"], pr["k_postfactor"], pr["k_postdraw"], pr["k_posterior"]
        print(f"medgp_posterior_joint_batch, {name}: wall {wall * 1e3:.1f} ms ({wall / wall_m:.1f} x the marginals' call); "
              f"k_posterior {kp[0]:.3f} ms ({kp[1]}); k_postcov {kc[0]:.3f} ms ({kc[1]}); k_postfactor {kf[0]:.3f} ms ({kf[1]}); "
              f"k_postdraw {kd[0]:.3f} ms ({kd[1]})")
        print(f"    k_postcov: m^2 n + pairs = {flop:.3e} flop -> {flop / (kc[0] * 1e-3) / 1e12:.2f} TFLOP/s = "
              f"{100 * flop / (kc[0] * 1e-3) / PEAK:.1f} % of fp64 peak", flush=True)
    if a.no_alt:
        return
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from posterior_joint_ref import draw, restate_joint  # noqa: E402
    ap_ = min(a.alt_patients, P)
    t0 = time.perf_counter()
    fac, st = ctx.factor_batch(slots, th, [N] * P)
    wall_f = time.perf_counter() - t0
    t0 = time.perf_counter()
    for p in range(ap_):
        ref = restate_joint(7, Q, D, R, *pts[p], th[p], m2s[p], t2s[p])
        draw(ref, eps[p])
    wall_n = (time.perf_counter() - t0) * P / ap_
    print(f"alternative: medgp_factor_batch wall {wall_f * 1e3:.1f} ms + numpy restatement {wall_n * 1e3:.0f} ms for {P} patients "
          f"(measured on {ap_}, {os.cpu_count()} cores visible, OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS')})")
    ctx.close()


if __name__ == "__main__":
    main()
