"""The inputs of the functional GPU tests (test_functional_gpu.py), built without a device so that the CPU suite (test_functional.py)
can vouch for the reference on exactly those inputs: on every one of them the fp64 restatement (functional_ref.restate) must agree with
the long-double one far inside the bar the device is held to.  The reference of a patient is computed once per process and shared.

The shapes are the smallest that reach each path of k_functional / medgp_functional_batch: n under one 64-row panel, on and around its
edge and over several panels; functional counts on and around the 64-column tile; term counts 0, 1, 2, 25 and 70 inside one tile, with
zero and negative weights; Q <= 8 and Q = 17; the three covariance families; every factorisation route.  A patient's functionals cycle
through the seven kinds of mix(): what a caller asks for (points, 24 h means, 6 h and 0.25 h changes, contrasts) next to 70 random terms
and the empty functional."""
import functools

import numpy as np

from medgp_amd import functionals as FN
from medgp_amd import synth
import functional_ref as FR
import trend_cases as TC

KINDS = 7
EDGE_COUNTS = (0, 1, 63, 64, 65, 130)
# name -> (kernel, Q, D, R, seed, sizes, functional counts, interleave), as trend_cases.CASES; a count of None: no functionals, no reference
CASES = {
    "parity_d3": (7, 3, 3, 2, 21, (70, 131, 5, 200), (36, 36, 36, 36), True),
    "parity_d24": (7, 5, 24, 8, 22, (300, 97), (36, 36), True),
    # ONE patient (n = 120) in six slots, a different functional count each
    "tile_edges": (7, 2, 3, 2, 23, (120,) * len(EDGE_COUNTS), EDGE_COUNTS, False),
    "q17": (7, 17, 2, 1, 46, (90, 150), (36, 36), False),
    "se": (0, 1, 1, 0, 47, (80, 140), (36, 36), False),
    "sm": (8, 3, 1, 0, 47, (80, 140), (36, 36), False),
    # the mix and, behind it, three contrasts of a point with itself
    "degenerate": (7, 3, 3, 2, 26, (131,), (36,), False),
    "routes": TC.CASES["routes"][:6] + (tuple(14 if p in TC.ROUTE_CHECKED else None for p in range(len(TC.ROUTE_SIZES))), False),
    "multi_cu": TC.CASES["multi_cu"][:6] + ((36, 36), False),
    "jitter": TC.CASES["jitter"][:6] + ((36, 36), False),
    "bits": TC.CASES["bits"][:6] + ((70, 100), False),
}
SAME_PATIENT = ("tile_edges",)
N_DEGENERATE = 3
JITTER_ROUNDS = TC.JITTER_ROUNDS
ROUTE_CHECKED = TC.ROUTE_CHECKED
fam_args = TC.fam_args


def mix(seed, D, t, count):
    """count functionals over the patient's time range (and a little beyond), kind j % 7 of
        0 a point                         1 the mean over 24 h, 25 Gauss-Legendre nodes      2 the change over 6 h
        3 the change over 0.25 h          4 covariate m against covariate m + 1 at one time (D = 1: the same covariate 12 h apart)
        5 70 random terms, normal weights (negative ones, and one exactly zero)             6 no term at all"""
    g = np.random.default_rng(seed)
    lo, hi = float(t.min()), float(t.max())
    out = []
    for j in range(count):
        kind = j % KINDS
        m = int(g.integers(0, D))
        tt = float(np.float32(g.uniform(lo - 3.0, hi + 3.0)))
        t0 = float(np.float32(g.uniform(lo - 3.0, max(hi - 21.0, lo))))
        if kind == 0:
            out.append(FN.point(m, tt))
        elif kind == 1:
            out.append(FN.window_mean(m, t0, t0 + 24.0, 25))
        elif kind == 2:
            out.append(FN.change(m, t0, t0 + 6.0))
        elif kind == 3:
            out.append(FN.change(m, t0, t0 + 0.25))
        elif kind == 4:
            out.append(FN.contrast((m, tt), ((m + 1) % D, tt)) if D > 1 else FN.contrast((0, tt), (0, tt + 12.0)))
        elif kind == 5:
            a = g.standard_normal(70)
            a[3] = 0.0
            out.append((g.integers(0, D, size=70).astype(np.int32), g.uniform(lo - 3.0, hi + 3.0, size=70).astype(np.float32), a))
        else:
            out.append((np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0)))
    return out


@functools.lru_cache(maxsize=None)
def case_lists(name):
    """the functionals of every patient of CASES[name] as a list of (meta2, t2, weight), or None; treat as read-only"""
    kidx, Q, D, R, seed, sizes, nfun, inter = CASES[name]
    _, pts, _, _ = _case_base(name)
    out = []
    for p, k in enumerate(nfun):
        if k is None:
            out.append(None)
            continue
        fs = mix(1000 * seed + p, D, pts[p][1], k)
        if name == "degenerate":
            g = np.random.default_rng(seed)
            for _ in range(N_DEGENERATE):
                pt = (int(g.integers(0, D)), float(g.uniform(20.0, 180.0)))
                fs.append(FN.contrast(pt, pt))
        out.append(fs)
    return out


@functools.lru_cache(maxsize=None)
def _case_base(name):
    kidx, Q, D, R, seed, sizes, nfun, inter = CASES[name]
    same = name in SAME_PATIENT
    pts = [synth.patient(seed, 0 if same else p, D, n, interleave=inter) for p, n in enumerate(sizes)]
    th = np.stack([synth.theta(seed, 0 if same else p, kidx, Q, D, R) for p in range(len(sizes))])
    return (kidx, Q, D, R), pts, th, None


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(family, patients [(meta, t, y)], theta [P, H], packed [(toffsets, meta2, t2, weight) or None]) of CASES[name]; read-only"""
    fam, pts, th, _ = _case_base(name)
    return fam, pts, th, [None if fs is None else FN.pack(fs) for fs in case_lists(name)]


def checked(name):
    """the patients of a case that have functionals (and a reference)"""
    return [p for p, k in enumerate(CASES[name][6]) if k is not None]


def restate(fam, pt, th, packed, jitter_rounds=0, dtype=np.float64):
    toff, m2, t2, a = packed
    return FR.restate(*fam_args(fam, pt), th, toff, m2 if fam[0] == 7 else None, t2, a, jitter_rounds, dtype)


@functools.lru_cache(maxsize=None)
def case_ref(name, p, dtype=np.float64):
    """functional_ref.restate of patient p of CASES[name] (computed once, shared by the tests; treat as read-only)"""
    fam, pts, th, qs = case_data(name)
    return restate(fam, pts[p], th[p], qs[p], JITTER_ROUNDS.get(name, 0), dtype)


EMPTY = (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0))


def call_list(qs, sel=None):
    """packed_list of Context.functionals for the patients sel (all by default); a patient without functionals gets the empty list"""
    sel = range(len(qs)) if sel is None else sel
    return [qs[p] if qs[p] is not None else EMPTY for p in sel]


@functools.lru_cache(maxsize=None)
def far_case():
    """(family, patient, theta, packed, q_g [F]) on trend_cases.far_case: points, a contrast, a 6 h change and a 24 h mean at
    t_max + 5000 h and t_min - 5000 h, where the envelope exp(-c_q tau^2) of every component towards the data has underflowed: the
    posterior of the functional is its prior"""
    fam, pt, th, (m2, t2), _ = TC.far_case()
    D = fam[2]
    hi, lo = float(t2[0]), float(t2[D])
    fs = [FN.point(int(m), float(t)) for m, t in zip(m2, t2)]
    fs += [FN.contrast((0, hi), (1, hi + 1.0)), FN.change(2, lo - 6.0, lo), FN.window_mean(1, hi, hi + 24.0, 25)]
    packed = FN.pack(fs)
    return fam, pt, th, packed, restate(fam, pt, th, packed)[2]
