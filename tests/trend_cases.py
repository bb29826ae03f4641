"""The inputs of the trend GPU tests (test_trend_gpu.py), built without a device so that the CPU suite (test_trend.py) can vouch for
the reference on exactly those inputs: on every one of them the fp64 restatement (trend_ref.restate) must agree with the
long-double one far inside the bar the device is held to.  The reference of a patient is computed once per process and shared.

The shapes are the smallest that reach each path of k_trend / medgp_trend_batch: n on and around the 64-row panel edge and over
several panels, point counts on and around the 32-point tile edge (and the 64 of the posterior call), Q <= 8 (tables) and Q = 17
(generic loop), the three covariance families, every factorisation route."""
import functools

import numpy as np

from medgp_amd import synth
import trend_ref as TR

# name -> (kernel, Q, D, R, seed, sizes, point counts, interleave); patient p of a case is synth.patient(seed, p, D, sizes[p]) with
# hypers synth.theta(seed, p, ...), its points points(1000 * seed + p, ...).  A point count of None: the patient gets no points and
# no reference (batch-mates that only fill a size class).
ROUTE_SIZES = [1000] + [330] * 200 + [60] * 4      # the composition of test_posterior_gpu.test_routes_all_three_and_pinned
ROUTE_CHECKED = [0, 1, 200, 201, 204]
EDGE_COUNTS = (0, 1, 31, 32, 33, 63, 64, 65, 200)
CASES = {
    "parity_d3": (7, 3, 3, 2, 21, (70, 131, 5, 200), (40, 70, 9, 1), True),
    "parity_d24": (7, 5, 24, 8, 22, (300, 97, 512), (130, 24, 64), True),
    # ONE patient (n = 120) in nine slots, a different point count each
    "tile_edges": (7, 2, 3, 2, 23, (120,) * len(EDGE_COUNTS), EDGE_COUNTS, False),
    "generic_q17": (7, 17, 2, 1, 46, (90, 150), (50, 50), False),
    "se": (0, 1, 1, 0, 47, (80, 140), (66, 66), False),
    "sm": (8, 3, 1, 0, 47, (80, 140), (66, 66), False),
    "routes": (7, 2, 2, 2, 44, tuple(ROUTE_SIZES), tuple(70 if p in ROUTE_CHECKED else None for p in range(len(ROUTE_SIZES))), False),
    "multi_cu": (7, 3, 4, 2, 45, (140, 250), (90, 90), False),
    "jitter": (7, 3, 3, 2, 24, (70, 131), (40, 40), False),
    "bits": (7, 3, 5, 2, 49, (150, 300), (100, 150), False),
}
JITTER_ROUNDS = {"jitter": 2}
FAR_H = 5000.0


def points(seed, D, t, m):
    """m test points: random covariates, times over the patient's range and a little beyond"""
    g = np.random.default_rng(seed)
    return (g.integers(0, D, size=m).astype(np.int32),
            g.uniform(float(t.min()) - 3.0, float(t.max()) + 3.0, size=m).astype(np.float32))


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(family, patients [(meta, t, y)], theta [P, H], points [(meta2, t2) or None]) of CASES[name]; treat as read-only"""
    kidx, Q, D, R, seed, sizes, npts, inter = CASES[name]
    same = name == "tile_edges"
    pts = [synth.patient(seed, 0 if same else p, D, n, interleave=inter) for p, n in enumerate(sizes)]
    th = np.stack([synth.theta(seed, 0 if same else p, kidx, Q, D, R) for p in range(len(sizes))])
    qs = [None if k is None else points(1000 * seed + p, D, pts[p][1], k) for p, k in enumerate(npts)]
    return (kidx, Q, D, R), pts, th, qs


def checked(name):
    """the patients of a case that have points (and a reference)"""
    return [p for p, k in enumerate(CASES[name][6]) if k is not None]


def fam_args(fam, pt):
    kidx, Q, D, R = fam
    return (kidx, Q, D, R, pt[0] if kidx == 7 else None, pt[1], pt[2])


@functools.lru_cache(maxsize=None)
def case_ref(name, p, dtype=np.float64):
    """trend_ref.restate of patient p of CASES[name] (computed once, shared by the tests; treat as read-only)"""
    fam, pts, th, qs = case_data(name)
    m2, t2 = qs[p]
    return TR.restate(*fam_args(fam, pts[p]), th[p], m2 if fam[0] == 7 else None, t2, JITTER_ROUNDS.get(name, 0), dtype)


def call_lists(fam, qs, sel=None):
    """(meta2_list or None, t2_list) of Context.trend for the patients sel (all by default); a patient without points gets none"""
    sel = range(len(qs)) if sel is None else sel
    e = (np.zeros(0, np.int32), np.zeros(0, np.float32))
    got = [qs[p] if qs[p] is not None else e for p in sel]
    return ([g[0] for g in got] if fam[0] == 7 else None), [g[1] for g in got]


@functools.lru_cache(maxsize=None)
def far_case():
    """(family, patient, theta, (meta2, t2), prior_dvar): every covariate at t_max + FAR_H and t_min - FAR_H, where the envelope
    exp(-c_q tau^2) of every component has underflowed: the posterior of the slope is its prior"""
    kidx, Q, D, R = fam = (7, 3, 3, 2)
    pt = synth.patient(25, 0, D, 100)
    th = synth.theta(25, 0, kidx, Q, D, R)
    t = pt[1]
    m2 = np.tile(np.arange(D, dtype=np.int32), 2)
    t2 = np.repeat(np.array([float(t.max()) + FAR_H, float(t.min()) - FAR_H], np.float32), D)
    _, B, w, c = TR.hypers(kidx, Q, D, R, th)
    prior = sum(B[q][m2, m2] * (w[q] * w[q] + 2.0 * c[q]) for q in range(Q))
    return fam, pt, th, (m2, t2), prior
