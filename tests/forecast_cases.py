"""The inputs of the forecast GPU tests (test_forecast_gpu.py), built from random_patients.py without a device so that the CPU
suite (test_forecast.py) can assert the condition the error bars rest on, cond(K) <= 1e6, and hold the one-factor identity
against the refit on every one of them.  The reference of a case (forecast_ref.refit) is computed once per process and shared.

The shapes are the smallest at which k_forecast can still go wrong: n and the prefixes sit on and around the 64-row panel
edges, the point counts on and around the 64-column tile edge."""
import functools

import numpy as np

from medgp_amd import synth
from random_patients import random_patient
import forecast_ref as FR

SEED = 20261018

# (kernel, Q, D, R, [(n, m, order, prefixes) per patient]): the three families; Q = 1, 5 separable, 9 generic, 17 generic with the
# Q > 16 assembly; D in {1, 2, 24, 64}; n in {1, 2, 63, 64, 65, 130, 300}; m in {0, 1, 64, 65, 200}.
#   order    'time'     uploaded sorted by time, covariates interleaved (the caller-order copy when D > 1)
#            'grouped'  uploaded grouped by covariate (the permutation is the identity)
#   prefixes 'mix'      {0, 1, 63, 64, 65, 127, 128, n - 1, n} within [0, n], then random ones, shuffled
#            'zeros'    all 0 (tiles that touch no panel)
#            'ends'     0 and n alternating (one tile mixing the prior and full conditioning)
#            'zhead'    70 points of prefix 0, then 'mix': a tile of zeros and a tile that mixes 0 with the rest
CASES = [
    (7, 5, 24, 8, [(300, 200, "time", "mix"), (130, 65, "grouped", "mix"), (65, 64, "time", "ends"), (64, 64, "grouped", "zeros"),
                   (63, 0, "time", "mix"), (2, 65, "time", "mix"), (1, 1, "grouped", "mix")]),
    (7, 1, 2, 1, [(130, 200, "time", "zhead"), (64, 65, "time", "mix"), (300, 64, "grouped", "mix")]),
    (7, 9, 1, 1, [(65, 65, "time", "mix"), (130, 64, "time", "ends"), (2, 1, "time", "mix")]),
    (7, 17, 2, 1, [(130, 65, "time", "mix"), (63, 64, "grouped", "mix"), (1, 1, "time", "mix")]),
    (7, 3, 64, 2, [(300, 65, "time", "mix"), (63, 200, "time", "mix")]),
    (8, 5, 1, 0, [(300, 200, "time", "zhead"), (64, 64, "time", "mix"), (2, 1, "time", "mix")]),
    (8, 9, 1, 0, [(130, 65, "time", "mix"), (65, 1, "time", "mix")]),
    (0, 1, 1, 0, [(130, 200, "time", "mix"), (1, 64, "time", "ends"), (63, 65, "time", "mix")]),
]


def case_id(s):
    return f"k{s[0]}Q{s[1]}D{s[2]}_" + "-".join(f"{n}x{m}{o[0]}{p[0]}" for n, m, o, p in s[4])


def patient(g, D, n, order):
    """(meta, t, y) in the order it is uploaded"""
    meta, t, y = random_patient(g, D, n, "plain")
    if order == "time":
        p = np.argsort(t, kind="stable")
        meta, t, y = meta[p], t[p], y[p]
    return meta, t, y


def _mix(g, n, m):
    special = np.array(sorted({p for p in (0, 1, 63, 64, 65, 127, 128, n - 1, n) if 0 <= p <= n}), np.int32)
    if m <= special.shape[0]:
        return g.choice(special, size=m, replace=False).astype(np.int32)
    return g.permutation(np.concatenate([special, g.integers(0, n + 1, size=m - special.shape[0]).astype(np.int32)])).astype(np.int32)


def prefixes(g, n, m, scheme):
    if scheme == "mix":
        return _mix(g, n, m)
    if scheme == "zeros":
        return np.zeros(m, np.int32)
    if scheme == "ends":
        return np.where(np.arange(m) % 2 == 0, 0, n).astype(np.int32)
    if scheme == "zhead":
        return g.permutation(np.concatenate([np.zeros(70, np.int32), _mix(g, n, m - 70)])).astype(np.int32)
    raise ValueError(scheme)


def points(g, D, t, m):
    """m test points: random covariates, times over the patient's range and a little beyond, observed values"""
    return (g.integers(0, D, size=m).astype(np.int32),
            g.uniform(float(t.min()) - 3.0, float(t.max()) + 3.0, size=m).astype(np.float32),
            g.standard_normal(m).astype(np.float32))


@functools.lru_cache(maxsize=None)
def case_data(i):
    """(family, patients [(meta, t, y)], theta [P, H], points [(meta2, t2, y2, prefix)]) of CASES[i]; treat as read-only"""
    kidx, Q, D, R, spec = CASES[i]
    g = np.random.Generator(np.random.Philox(key=[SEED, i]))
    pts = [patient(g, D, n, order) for n, _, order, _ in spec]
    th = np.stack([synth.theta(SEED + i, p, kidx, Q, D, R) for p in range(len(spec))])
    qs = [points(g, D, pt[1], m) + (prefixes(g, n, m, scheme),) for pt, (n, m, _, scheme) in zip(pts, spec)]
    return (kidx, Q, D, R), pts, th, qs


def fam_args(fam, pt):
    kidx, Q, D, R = fam
    return (kidx, Q, D, R, pt[0] if kidx == 7 else None, pt[1], pt[2])


@functools.lru_cache(maxsize=None)
def case_ref(i, p, jitter_rounds=0):
    """forecast_ref.refit of patient p of CASES[i] (computed once, shared by the tests; treat as read-only)"""
    fam, pts, th, qs = case_data(i)
    m2, t2, y2, pf = qs[p]
    return FR.refit(*fam_args(fam, pts[p]), th[p], m2 if fam[0] == 7 else None, t2, pf, y2, jitter_rounds=jitter_rounds)


def call_lists(fam, qs, sel=None):
    """(meta2_list or None, t2_list, prefix_list, y2_list) of Context.forecast for the patients sel (all by default)"""
    sel = range(len(qs)) if sel is None else sel
    return ([qs[p][0] for p in sel] if fam[0] == 7 else None, [qs[p][1] for p in sel], [qs[p][3] for p in sel], [qs[p][2] for p in sel])
