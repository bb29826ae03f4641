"""The inputs of the components GPU tests (test_components_gpu.py), built without a device so that the CPU suite (test_components.py)
can vouch for the reference on exactly those inputs: on every one of them the fp64 restatement (components_ref.restate) must agree
with the long-double one far inside the bar the device is held to.  The reference of a patient is computed once per process and shared.

The shapes are the smallest that reach each path of k_components / medgp_components_batch: n on and around the 64-row panel edge and
over several panels; point counts on and around the tile width P = 64 / Q for a P that is a power of two (Q = 2) and one that is not
(Q = 3); Q = 17 (three points and thirteen dead columns per tile) and Q = 64 (one point per tile, 2016 pairs: eight per thread);
Q = 1 (SE: no pair at all); the three covariance families; every factorisation route."""
import functools

import numpy as np

from medgp_amd import synth
import components_ref as CR
import trend_cases as TC
import trend_ref as TR

EDGE_COUNTS_Q3 = (0, 1, 20, 21, 22, 42, 43, 64, 65, 200)
EDGE_COUNTS_Q2 = (31, 32, 33)
# name -> (kernel, Q, D, R, seed, sizes, point counts, interleave), as trend_cases.CASES
CASES = {
    "parity_d3": (7, 3, 3, 2, 21, (70, 131, 5, 200), (40, 70, 9, 1), True),
    "parity_d24": (7, 5, 24, 8, 22, (300, 97, 512), (130, 24, 64), True),
    # ONE patient (n = 120) in ten / three slots, a different point count each
    "tile_edges_q3": (7, 3, 3, 2, 23, (120,) * len(EDGE_COUNTS_Q3), EDGE_COUNTS_Q3, False),
    "tile_edges_q2": (7, 2, 3, 2, 23, (120,) * len(EDGE_COUNTS_Q2), EDGE_COUNTS_Q2, False),
    "q17": (7, 17, 2, 1, 46, (90, 150), (50, 50), False),
    "q64": (7, 64, 2, 1, 48, (90,), (5,), False),
    "se": (0, 1, 1, 0, 47, (80, 140), (66, 66), False),
    "sm": (8, 3, 1, 0, 47, (80, 140), (66, 66), False),
    "routes": TC.CASES["routes"],
    "multi_cu": TC.CASES["multi_cu"],
    "jitter": TC.CASES["jitter"],
    "bits": TC.CASES["bits"],
}
SAME_PATIENT = ("tile_edges_q3", "tile_edges_q2")
JITTER_ROUNDS = TC.JITTER_ROUNDS
ROUTE_CHECKED = TC.ROUTE_CHECKED
points, fam_args, call_lists = TC.points, TC.fam_args, TC.call_lists


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(family, patients [(meta, t, y)], theta [P, H], points [(meta2, t2) or None]) of CASES[name]; treat as read-only"""
    kidx, Q, D, R, seed, sizes, npts, inter = CASES[name]
    same = name in SAME_PATIENT
    pts = [synth.patient(seed, 0 if same else p, D, n, interleave=inter) for p, n in enumerate(sizes)]
    th = np.stack([synth.theta(seed, 0 if same else p, kidx, Q, D, R) for p in range(len(sizes))])
    qs = [None if k is None else points(1000 * seed + p, D, pts[p][1], k) for p, k in enumerate(npts)]
    return (kidx, Q, D, R), pts, th, qs


def checked(name):
    """the patients of a case that have points (and a reference)"""
    return [p for p, k in enumerate(CASES[name][6]) if k is not None]


@functools.lru_cache(maxsize=None)
def case_ref(name, p, dtype=np.float64):
    """components_ref.restate of patient p of CASES[name] (computed once, shared by the tests; treat as read-only)"""
    fam, pts, th, qs = case_data(name)
    m2, t2 = qs[p]
    return CR.restate(*fam_args(fam, pts[p]), th[p], m2 if fam[0] == 7 else None, t2, JITTER_ROUNDS.get(name, 0), dtype)


@functools.lru_cache(maxsize=None)
def far_case():
    """(family, patient, theta, (meta2, t2), prior [m, Q]) of trend_cases.far_case: every covariate at t_max + 5000 h and
    t_min - 5000 h, where the envelope exp(-c_q tau^2) of every component has underflowed: the posterior of a component is its prior"""
    fam, pt, th, (m2, t2), _ = TC.far_case()
    _, B, _, _ = TR.hypers(*fam, th)
    return fam, pt, th, (m2, t2), np.stack([B[q][m2, m2] for q in range(fam[1])], axis=1)
