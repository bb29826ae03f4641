"""The inputs of the leave-one-out GPU tests (test_loo_gpu.py), built without a device so that the CPU suite (test_loo.py)
can assert the condition the error bars rest on, cond(K) <= 1e4, and the agreement of the two restatements for every one of
them.  The reference of a case (loo_ref.refit) is computed once per process and shared."""
import functools

import numpy as np

from medgp_amd import synth
import loo_ref

# (kernel, Q, D, R, n per patient, grouping scheme): the three families, separable (Q <= 8) and generic (Q = 9, 17) kernels,
# D in {1, 3, 24, 64}, n in {1, 2, 3, 63, 64, 65, 130, 300} ragged in one call.  Schemes:
#   null       every observation its own group (group = NULL)
#   covariate  the patient's meta, D groups (D = 64 with n = 63, D = 24 with n = 3: unobserved covariates = empty groups)
#   window     24-hour windows of the observation times
#   random5    5 random groups
#   all        one group of everything (sizes 1, 2, 3, 63, 64, 65, 130, 300: the 64-row panel edges of the block kernels)
#   minus      5 random groups with a third of the observations never held out (-1)
#   mixed      singletons next to larger groups in one patient, ids shuffled over the observations
CASES = [
    (7, 3, 3, 2, (1, 2, 3, 63, 64, 65, 130, 300), "null"),
    (7, 3, 3, 2, (1, 2, 3, 63, 64, 65, 130, 300), "all"),
    (7, 5, 24, 8, (300, 130, 65, 3), "covariate"),
    (7, 2, 64, 2, (130, 63, 300), "covariate"),
    (7, 8, 3, 2, (300, 65, 2), "window"),
    (7, 9, 3, 1, (130, 64, 3), "random5"),
    (7, 17, 1, 1, (65, 130, 1), "minus"),
    (7, 3, 24, 4, (130, 300, 63), "mixed"),
    (8, 3, 1, 0, (300, 63, 2), "mixed"),
    (8, 9, 1, 0, (64, 130), "window"),
    (0, 1, 1, 0, (130, 1, 65), "random5"),
    (0, 1, 1, 0, (64, 300, 3), "minus"),
    (0, 1, 1, 0, (65, 2, 130), "covariate"),
]


def case_id(s):
    return f"k{s[0]}Q{s[1]}D{s[2]}_n{'-'.join(map(str, s[4]))}_{s[5]}"


def grouping(scheme, g, kidx, D, pt):
    """(group ids or None, ngroups or None) of one patient under a scheme"""
    meta, t, _ = pt
    n = t.shape[0]
    if scheme == "null":
        return None, None
    if scheme == "covariate":
        return (meta.astype(np.int32), D) if kidx == 7 else (np.zeros(n, np.int32), 1)
    if scheme == "window":
        ids = np.floor(t.astype(np.float64) / 24.0).astype(np.int32)
        return ids, int(ids.max()) + 1
    if scheme == "random5":
        return g.integers(0, 5, size=n).astype(np.int32), 5
    if scheme == "all":
        return np.zeros(n, np.int32), 1
    if scheme == "minus":
        ids = g.integers(0, 5, size=n).astype(np.int32)
        ids[g.random(n) < 1.0 / 3.0] = -1
        return ids, 5
    if scheme == "mixed":
        # the first half singletons, then groups of 2, 70 (where there are that many) and the rest
        ids = np.arange(n, dtype=np.int32)
        a = n // 2
        for size in (2, 70, n):
            e = min(a + size, n)
            if e <= a:
                break
            ids[a:e] = a
            a = e
        _, ids = np.unique(ids, return_inverse=True)
        return ids.astype(np.int32)[g.permutation(n)], int(ids.max()) + 1
    raise ValueError(scheme)


@functools.lru_cache(maxsize=None)
def case_data(i):
    """(patients, theta, [group ids or None per patient], [number of groups per patient]) of CASES[i]"""
    kidx, Q, D, R, ns, scheme = CASES[i]
    pts = [synth.patient(7100 + i, p, D, n, interleave=(p % 2 == 1)) for p, n in enumerate(ns)]
    th = np.stack([synth.theta(7100 + i, p, kidx, Q, D, R) for p in range(len(ns))])
    g = np.random.Generator(np.random.Philox(key=[7100, i]))
    gr = [grouping(scheme, g, kidx, D, pt) for pt in pts]
    # a list of ids handed to Context.loo is sized by its largest id: the same count here (trailing empty groups only exist by covariate)
    # (no ids: every observation its own group, n groups)
    ngs = [pt[1].shape[0] if x[0] is None else x[1] if scheme == "covariate" else (int(x[0].max()) + 1 if x[0].size and x[0].max() >= 0 else 0)
           for x, pt in zip(gr, pts)]
    return pts, th, [x[0] for x in gr], ngs


def call_groups(i):
    """the `groups` argument of Context.loo for CASES[i]"""
    _, _, gs, _ = case_data(i)
    if CASES[i][5] == "null":
        return None
    if CASES[i][5] == "covariate":
        return "covariate"
    return gs


def family_args(fam, pt):
    kidx, Q, D, R = fam
    return (kidx, Q, D, R, pt[0] if kidx == 7 else None, pt[1], pt[2])


@functools.lru_cache(maxsize=None)
def case_ref(i, p, jitter_rounds=0):
    """loo_ref.refit of patient p of CASES[i] (computed once, shared by the tests; treat as read-only)"""
    pts, th, gs, ngs = case_data(i)
    return loo_ref.refit(*family_args(CASES[i][:4], pts[p]), th[p], gs[p], ngs[p], jitter_rounds=jitter_rounds)


def jitter_case():
    """four patients of three size classes, by 24-hour window and (patient 3) interleaved"""
    fam = (7, 3, 3, 2)
    ns = (40, 300, 64, 150)
    pts = [synth.patient(7300, p, fam[2], n, interleave=(p == 3)) for p, n in enumerate(ns)]
    th = np.stack([synth.theta(7300, p, *fam) for p in range(len(ns))])
    g = np.random.Generator(np.random.Philox(key=[7300, 0]))
    gs = [grouping("window" if p != 2 else "mixed", g, fam[0], fam[2], pt)[0] for p, pt in enumerate(pts)]
    return fam, pts, th, gs


def invariance_case():
    """two patients of one size class (so that a small budget cuts the class into launch chunks) and two of others"""
    fam = (7, 3, 5, 2)
    ns = (300, 290, 150, 64)
    pts = [synth.patient(7400, p, fam[2], n, interleave=(p == 1)) for p, n in enumerate(ns)]
    th = np.stack([synth.theta(7400, p, *fam) for p in range(len(ns))])
    g = np.random.Generator(np.random.Philox(key=[7400, 0]))
    gs = [grouping("random5", g, fam[0], fam[2], pt)[0] for pt in pts]
    return fam, pts, th, gs
