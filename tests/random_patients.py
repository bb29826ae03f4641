"""Seeded random patients for the GPU sweeps (test_fuzz_gpu.py: nlml + gradient, test_posterior_fuzz_gpu.py: posterior)."""
import numpy as np


def random_patient(g, D, n, mode):
    """(meta, t, y) in caller order. mode: 'plain' | 'missing' (some outputs never observed) | 'same_time' (one output observed
    only at ONE time stamp, several times) | 'shuffled' (not grouped by output) | 'burst' (all of it inside one hour)."""
    outs = np.arange(D)
    if mode == "missing" and D > 1:
        outs = np.sort(g.choice(D, size=max(1, D // 2), replace=False))
    m = np.sort(g.choice(outs, size=n)).astype(np.int32)
    span = 1.0 if mode == "burst" else 200.0
    t = g.uniform(0.0, span, size=n).astype(np.float32)
    if mode == "same_time" and n >= 6:
        d0 = m[0]
        sel = np.where(m == d0)[0][:3]
        t[sel] = t[sel[0]]
    for d in outs:                                   # the loader's order: sorted by time inside an output
        idx = np.where(m == d)[0]
        t[idx] = np.sort(t[idx])
    y = g.standard_normal(n).astype(np.float32)
    if mode == "shuffled":
        p = g.permutation(n)
        m, t, y = m[p], t[p], y[p]
    return m, t, y
