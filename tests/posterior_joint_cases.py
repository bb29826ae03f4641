"""The inputs of the joint-posterior GPU tests (test_posterior_joint_gpu.py), built without a device so that the CPU suite
(test_posterior_joint.py) can assert the condition the error bar rests on, cond(C) <= 1e4, for every one of them."""
import functools

import numpy as np

from medgp_amd import synth

# (kernel, Q, D, R, n per patient, m per patient, nsamp, cov): the three families, separable (Q <= 8) and generic (Q = 9, 17)
# kernels, D from 1 to 64, n in {1, 2, 63, 64, 65, 300}, m in {0, 1, 63, 64, 65, 130, 700}, ragged m in one call
SHAPES = [
    (7, 3, 3, 2, (1, 2, 63, 64, 65, 300), (0, 1, 63, 64, 65, 130), 7, True),
    (7, 5, 24, 8, (300, 64, 65), (700, 130, 1), 64, True),
    (7, 8, 4, 2, (65, 300, 2), (64, 130, 63), 1, True),
    (7, 9, 2, 1, (63, 300), (65, 130), 1, True),
    (7, 17, 1, 1, (64, 300, 2), (64, 63, 0), 7, False),
    (7, 2, 64, 2, (300, 65), (130, 64), 0, True),
    (8, 3, 1, 0, (1, 300, 63), (65, 700, 0), 7, True),
    (8, 9, 1, 0, (300, 64), (130, 65), 64, False),
    (0, 1, 1, 0, (2, 300, 64), (130, 63, 1), 64, True),
    (0, 1, 1, 0, (300, 65), (700, 64), 0, True),
]


def shape_id(s):
    return f"k{s[0]}Q{s[1]}D{s[2]}_n{'-'.join(map(str, s[4]))}_m{'-'.join(map(str, s[5]))}_s{s[6]}{'_cov' if s[7] else ''}"


def grid(g, D, m):
    """m test points: random covariates, times over the 200 h window of synth.patient and 3 h beyond"""
    return g.integers(0, D, size=m).astype(np.int32), g.uniform(-3.0, 203.0, size=m).astype(np.float32)


def normals(g, m, nsamp):
    return g.standard_normal((m, nsamp))


@functools.lru_cache(maxsize=None)
def shape_data(i):
    """(patients, theta, test points, eps or None) of SHAPES[i]"""
    kidx, Q, D, R, ns, ms, nsamp, _ = SHAPES[i]
    pts = [synth.patient(6100 + i, p, D, n, interleave=(p % 2 == 1)) for p, n in enumerate(ns)]
    th = np.stack([synth.theta(6100 + i, p, kidx, Q, D, R) for p in range(len(ns))])
    g = np.random.Generator(np.random.Philox(key=[6100, i]))
    tp = [grid(g, D, m) for m in ms]
    eps = [normals(g, m, nsamp) for m in ms] if nsamp else None
    return pts, th, tp, eps


def duplicates_case():
    """one patient whose test points hold ten exact duplicates and ten copies of training points"""
    kidx, Q, D, R, n, m = 7, 4, 6, 3, 200, 150
    pt = synth.patient(6200, 0, D, n, interleave=True)
    th = synth.theta(6200, 0, kidx, Q, D, R)
    g = np.random.Generator(np.random.Philox(key=[6200, 0]))
    m2, t2 = grid(g, D, m)
    src = g.choice(n, size=10, replace=False)
    m2[20:30], t2[20:30] = pt[0][src], pt[1][src]          # on training points
    m2[100:110], t2[100:110] = m2[40:50], t2[40:50]        # duplicated test points
    return (kidx, Q, D, R), pt, th, (m2, t2), normals(g, m, 7)


def jitter_case():
    kidx, Q, D, R = 7, 3, 3, 2
    ns, ms = (40, 300, 64, 150), (30, 130, 1, 65)
    pts = [synth.patient(6300, p, D, n, interleave=(p == 3)) for p, n in enumerate(ns)]
    th = np.stack([synth.theta(6300, p, kidx, Q, D, R) for p in range(len(ns))])
    g = np.random.Generator(np.random.Philox(key=[6300, 0]))
    tp = [grid(g, D, m) for m in ms]
    return (kidx, Q, D, R), pts, th, tp, [normals(g, m, 7) for m in ms]


def invariance_case():
    """two patients of one size class (so that a small budget cuts the class into launch chunks) and two of others"""
    kidx, Q, D, R = 7, 3, 5, 2
    ns, ms = (300, 290, 150, 64), (130, 100, 100, 65)
    pts = [synth.patient(6400, p, D, n) for p, n in enumerate(ns)]
    th = np.stack([synth.theta(6400, p, kidx, Q, D, R) for p in range(len(ns))])
    g = np.random.Generator(np.random.Philox(key=[6400, 0]))
    tp = [grid(g, D, m) for m in ms]
    return (kidx, Q, D, R), pts, th, tp, [normals(g, m, 7) for m in ms]
