"""Linear functionals of the latent function for Context.functionals / medgp_functional_batch (pure numpy; the posterior itself comes
from the device): builders of the term lists, the packing of many functionals into one call, and what a posterior says.

A functional is g = sum_k a_k f_{m_k}(t_k), written as three arrays (meta2 int32 [T], t2 float32 [T], weight float64 [T]): covariate,
time in hours and weight of every term.  Given the data g is Gaussian with the mean and variance the call returns (LATENT: no noise
term, include/medgp_hip.h).  The builders return such a triple; anything else that is linear in f -- a trapezoid rule, a difference of
two window means -- is the concatenation of triples with scaled weights (`combine`).
"""
import math

import numpy as np

_erfc = np.frompyfunc(math.erfc, 1, 1)


def _terms(m, t, a):
    return np.asarray(m, np.int32).ravel(), np.asarray(t, np.float32).ravel(), np.asarray(a, np.float64).ravel()


def point(m, t):
    """f_m(t): one term of weight 1 (the latent value the posterior call predicts, without the noise)"""
    return _terms([m], [t], [1.0])


def change(m, t0, t1):
    """f_m(t1) - f_m(t0): the change of covariate m from t0 to t1"""
    return _terms([m, m], [t1, t0], [1.0, -1.0])


def contrast(a, b):
    """f_m(t) - f_m'(t') for a = (m, t), b = (m', t'): is covariate m running above covariate m'"""
    return _terms([a[0], b[0]], [a[1], b[1]], [1.0, -1.0])


def window_mean(m, t0, t1, nodes):
    """(1 / (t1 - t0)) integral_{t0}^{t1} f_m(t) dt by Gauss-Legendre quadrature with `nodes` nodes: exact for polynomials of degree
    2 nodes - 1, the weights (already divided by t1 - t0) sum to 1.  The nodes are rounded to the float32 times the library takes."""
    nodes = int(nodes)
    if nodes < 1:
        raise ValueError(f"nodes = {nodes}")
    if not t1 > t0:
        raise ValueError(f"empty window [{t0}, {t1}]")
    x, w = np.polynomial.legendre.leggauss(nodes)
    return _terms(np.full(nodes, m), 0.5 * (t0 + t1) + 0.5 * (t1 - t0) * x, 0.5 * w)


def combine(parts, scales=None):
    """sum_i scales[i] parts[i] as one functional: the term lists concatenated in order, the weights scaled (scales None: all 1)"""
    parts = [_terms(*p) for p in parts]
    scales = [1.0] * len(parts) if scales is None else list(scales)
    if len(scales) != len(parts):
        raise ValueError(f"{len(scales)} scales for {len(parts)} functionals")
    if not parts:
        return _terms([], [], [])
    return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
            np.concatenate([s * p[2] for s, p in zip(scales, parts)]))


def pack(functionals):
    """One patient's list of functionals as the call takes them: (toffsets int64 [F + 1], meta2 int32 [T], t2 float32 [T], weight
    float64 [T]), functional f owning the terms [toffsets[f], toffsets[f + 1]).  A functional may have no terms."""
    fs = []
    for f, fn in enumerate(functionals):
        if len(fn) != 3:
            raise ValueError(f"functional {f}: expected (meta2, t2, weight)")
        m, t, a = _terms(*fn)
        if not (m.shape[0] == t.shape[0] == a.shape[0]):
            raise ValueError(f"functional {f}: {m.shape[0]} covariates, {t.shape[0]} times, {a.shape[0]} weights")
        fs.append((m, t, a))
    toff = np.zeros(len(fs) + 1, np.int64)
    if fs:
        toff[1:] = np.cumsum([f[0].shape[0] for f in fs])
    cat = (lambda k, dt: np.concatenate([f[k] for f in fs]).astype(dt) if fs else np.zeros(0, dt))
    return toff, cat(0, np.int32), cat(1, np.float32), cat(2, np.float64)


def prob_above(mean, var, threshold):
    """P(g > threshold) = Phi((mean - threshold) / sqrt(var)) under the posterior of the functional.  var == 0 (g known exactly) gives
    0, 1/2 or 1 by the sign of mean - threshold; NaN inputs (a failed patient) and var < 0 give NaN."""
    mu = np.asarray(mean, np.float64)
    v = np.asarray(var, np.float64)
    if mu.shape != v.shape:
        raise ValueError(f"mean has shape {mu.shape}, var {v.shape}")
    d = mu - np.asarray(threshold, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(v > 0, d / np.sqrt(np.where(v > 0, v, 1.0)), np.nan)
    exact = (v == 0) & ~np.isnan(d)
    u = np.where(exact, np.where(d > 0, np.inf, np.where(d < 0, -np.inf, 0.0)), u)
    p = 0.5 * np.asarray(_erfc(-u / math.sqrt(2.0)), np.float64)   # erfc: no cancellation in the lower tail
    return p.reshape(mu.shape)
