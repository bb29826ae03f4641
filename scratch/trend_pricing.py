"""k_trend priced beside k_posterior: the same points of the same build, 64 patients x N = 512, D = 24, Q = 5, 256 points each.
HIP-event time of every launch (medgp_profile_*), best of 5 calls after a warm-up.  Prints the record kept in
profiles/trend_pricing.txt:   python scratch/trend_pricing.py > profiles/trend_pricing.txt"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import medgp_amd
from medgp_amd import synth

P, N, D, Q, R, M = 64, 512, 24, 5, 8, 256
pts, th = synth.cohort(7, P, D, N, Q=Q, R=R)
ctx = medgp_amd.Context(7, Q, D, R)
ctx.reserve(P, N, P)
for s, (m, t, y) in enumerate(pts):
    ctx.set_patient(s, m, t, y)
g = np.random.default_rng(3)
m2s = [g.integers(0, D, size=M).astype(np.int32) for _ in range(P)]
t2s = [g.uniform(float(p[1].min()), float(p[1].max()), size=M).astype(np.float32) for p in pts]
slots = np.arange(P)


def price(fn, kernel):
    fn()
    best = None
    for _ in range(5):
        ctx.profile_reset()
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        prof = {k: v for k, v in ctx.profile_read().items() if v[1] > 0}
        if best is None or prof[kernel][0] < best[1][kernel][0]:
            best = (wall, prof)
    return best


ctx.profile_enable(True)
wt, pt_ = price(lambda: ctx.trend(slots, th, m2s, t2s), "k_trend")
wp, pp = price(lambda: ctx.posterior(slots, th, m2s, t2s, parts=False), "k_posterior")
fmt = lambda prof: "; ".join(f"{k} {v[0]:.3f} ms ({v[1]})" for k, v in prof.items())
a, b = ctx.trend(slots, th, m2s, t2s)[0], ctx.posterior(slots, th, m2s, t2s, parts=False)[0]
same = all(np.array_equal(a[p][k].view(np.uint32), b[p][k].view(np.uint32)) for p in range(P) for k in (0, 1))
lines = [
    "k_trend priced beside k_posterior (python scratch/trend_pricing.py; MI355X, one GPU, best of 5 calls after a warm-up; kernel times",
    "from HIP events around every launch, launches in parentheses)",
    "",
    f"case: {P} patients x N = {N}, D = {D}, Q = {Q}, {M} points each, the same points for both calls",
    f"medgp_trend_batch: wall {wt:.2f} ms; {fmt(pt_)}",
    f"medgp_posterior_batch(parts = NULL): wall {wp:.2f} ms; {fmt(pp)}",
    f"    k_trend / k_posterior = {pt_['k_trend'][0] / pp['k_posterior'][0]:.2f}   ({P * M // 32} tiles of 32 points against {P * M // 64} tiles of 64)",
    f"    mean / var of the two calls bitwise equal: {same}",
    f"    route(s) {ctx.last_plan()}",
]
print("\n".join(lines))
ctx.close()
