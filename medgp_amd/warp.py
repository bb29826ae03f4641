"""Learned output warping for skewed covariates: helpers around Context.warp_nlml_grad / Context.warp_posterior
(medgp_warp_nlml_grad, medgp_warp_posterior_batch).

A warped GP (Snelson, Rasmussen & Ghahramani 2004): z = g_d(y) is Gaussian under the GP, with the sinh-arcsinh map (Jones & Pewsey
2009) per covariate, psi_d = (a, eps, lambda), delta = exp(lambda):

    g(y) = a + sinh(delta asinh(y) - eps),   log g'(y) = lambda + log cosh(delta asinh(y) - eps) - log(1 + y^2) / 2,
    g^-1(z) = sinh((asinh(z - a) + eps) / delta)

psi = 0 is the identity; eps > 0 describes right-skewed data (y = g^-1(z) = sinh(asinh(z) + eps) has a long right tail), lambda sets
the tail weight (delta < 1: heavier tails than the normal).  A
covariate of kind NONE is left as it is.  Quantiles of a prediction are exact, g^-1(zmean + zq sd); its mean and variance in
observation space have no closed form: `moments` applies a Gauss-Hermite rule to zmean, zvar.  How good the rule is depends on the
tails of g^-1 AND on the predictive sd in z, so two figures that look far apart do not contradict each other: with the default 32
nodes the rule is good to about 1e-5 of the predictive sd for delta >= 1, and only to about 5e-4 at delta = 0.5 with a predictive sd
of 2 in z (both measured in numpy against a dense quadrature, on a wide prediction).  Over the case set of tests/warp_truth.py
tests/test_warp_truth.py measures 2.2e-7 for the mean and 3.1e-7 for the sd, relative to the predictive sd in observation space,
although delta goes down to 0.5 there: the predictive sd in z is at most 1.02 over the set (half of the 2 behind the 5e-4), and the
rule's error falls steeply with it -- the worst point of the set has delta >= 0.75, which is why the two entries of
warp_truth.MOMENTS_MEASURED coincide.  A forecast far from the data has the prior's sd: the first pair of figures applies there.
"""
import math
from statistics import NormalDist

import numpy as np

from .capi import KERNEL_LMC_SM

NONE, SAS = 0, 1
NPSI = 3


def identity(D):
    """psi [D, 3] of the identity map"""
    return np.zeros((D, NPSI))


def _rows(psi, kind, meta, D):
    """(a, eps, lambda, sas) per element of meta"""
    psi = np.asarray(psi, np.float64).reshape(D, NPSI)
    m = np.zeros(1, np.int64) if meta is None else np.asarray(meta, np.int64)
    sas = np.ones(D, bool) if kind is None else (np.asarray(kind).reshape(D) == SAS)
    return psi[m, 0], psi[m, 1], psi[m, 2], sas[m]


def _D(psi):
    return np.asarray(psi).size // NPSI


def forward(y, psi, kind=None, meta=None):
    """z = g_{meta}(y); psi [D, 3], kind [D] or None = all SAS, meta [n] or None = covariate 0"""
    y = np.asarray(y, np.float64)
    a, e, l, sas = _rows(psi, kind, meta, _D(psi))
    return np.where(sas, a + np.sinh(np.exp(l) * np.arcsinh(y) - e), y)


def inverse(z, psi, kind=None, meta=None):
    """y = g^-1_{meta}(z)"""
    z = np.asarray(z, np.float64)
    a, e, l, sas = _rows(psi, kind, meta, _D(psi))
    return np.where(sas, np.sinh((np.arcsinh(z - a) + e) / np.exp(l)), z)


def log_jacobian(y, psi, kind=None, meta=None):
    """log g'_{meta}(y)"""
    y = np.asarray(y, np.float64)
    a, e, l, sas = _rows(psi, kind, meta, _D(psi))
    u = np.abs(np.exp(l) * np.arcsinh(y) - e)
    return np.where(sas, l + (u + np.log1p(np.exp(-2 * u)) - math.log(2.0)) - 0.5 * np.log1p(y * y), 0.0)


def _sas_index(kind, D):
    return np.arange(D) if kind is None else np.flatnonzero(np.asarray(kind).reshape(D) == SAS)


def pack(theta, psi, kind=None):
    """the optimiser vector [theta | psi restricted to the SAS covariates] per patient: theta [nbatch, H], psi [nbatch, D, 3]"""
    theta = np.asarray(theta, np.float64)
    nb = theta.shape[0]
    psi = np.asarray(psi, np.float64).reshape(nb, -1, NPSI)
    idx = _sas_index(kind, psi.shape[1])
    return np.concatenate([theta, psi[:, idx, :].reshape(nb, -1)], axis=1)


def unpack(x, H, D, kind=None):
    """(theta [nbatch, H], psi [nbatch, D, 3]) of packed vectors; the rows of NONE covariates are 0"""
    x = np.asarray(x, np.float64)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    idx = _sas_index(kind, D)
    if x.shape[1] != H + NPSI * idx.shape[0]:
        raise ValueError(f"{x.shape[1]} values per patient, expected {H} + 3 x {idx.shape[0]}")
    psi = np.zeros((x.shape[0], D, NPSI))
    psi[:, idx, :] = x[:, H:].reshape(x.shape[0], idx.shape[0], NPSI)
    return x[:, :H].copy(), psi


def prior_grad(psi, mean=0.0, sd=1.0):
    """(-log density [..], its gradient shaped like psi) of independent Normal priors on a, eps and lambda (constants dropped).  The
    default N(0, 1) on each keeps delta near 1 where the data do not ask otherwise.  mean, sd: scalars or arrays that broadcast."""
    psi = np.asarray(psi, np.float64)
    r = (psi - mean) / sd
    return 0.5 * np.sum((r * r).reshape(*psi.shape[:-2], -1), axis=-1), r / sd


def objective(ctx, slots, kind=None, prior=None):
    """A closure x -> (values [nbatch], grads [nbatch, H + 3 #SAS]) over the packed vector [theta | psi of the SAS covariates] per
    patient, for an optimiser.  prior: None, or (mean, sd) of the Normal prior on psi that prior_grad adds (True: N(0, 1))."""
    slots = np.ascontiguousarray(slots, dtype=np.int32).ravel()
    nb = slots.shape[0]
    D = ctx.D if ctx.kernel_index == KERNEL_LMC_SM else 1
    idx = _sas_index(kind, D)
    pr = (0.0, 1.0) if prior is True else prior

    def f(x):
        th, psi = unpack(np.asarray(x, np.float64).reshape(nb, -1), ctx.H, D, kind)
        r = ctx.warp_nlml_grad(slots, th, psi, kind=kind)
        v, g = r["nlml"], np.concatenate([r["grad"], r["dpsi"][:, idx, :].reshape(nb, -1)], axis=1)
        if pr is not None:
            pv, pg = prior_grad(psi[:, idx, :], *pr)
            v = v + pv
            g[:, ctx.H:] += pg.reshape(nb, -1)
        return v, g
    return f


def init_from_moments(y, meta, D):
    """psi [D, 3] to start from: eps from the sample skewness of each covariate's values, with its sign (right-skewed data: eps > 0,
    so that g compresses the right tail), a and lambda at 0.  |eps| <= 1; fewer than three values or no spread: 0."""
    y = np.asarray(y, np.float64)
    m = np.zeros(y.shape[0], np.int64) if meta is None else np.asarray(meta, np.int64)
    psi = identity(D)
    for d in range(D):
        v = y[m == d]
        if v.shape[0] < 3 or v.std() == 0:
            continue
        c = v - v.mean()
        skew = np.mean(c ** 3) / v.std() ** 3
        psi[d, 1] = float(np.clip(skew / 2.0, -1.0, 1.0))
    return psi


def moments(zmean, zvar, psi, kind=None, meta2=None, nodes=32):
    """(mean, var) of the observed value at points whose z is N(zmean, zvar): the Gauss-Hermite rule with `nodes` nodes through g^-1.
    See the module docstring for how good the rule is."""
    zmean, zvar = np.asarray(zmean, np.float64), np.asarray(zvar, np.float64)
    x, w = np.polynomial.hermite_e.hermegauss(nodes)
    w = w / w.sum()
    zz = zmean[..., None] + np.sqrt(zvar)[..., None] * x
    mm = None if meta2 is None else np.asarray(meta2, np.int64)[..., None] * np.ones(nodes, np.int64)
    yy = inverse(zz, psi, kind, mm)
    mean = yy @ w
    return mean, ((yy - mean[..., None]) ** 2) @ w


def pit(y2, zmean, zvar, psi, kind=None, meta2=None):
    """the probability integral transform Phi((g(y2) - zmean) / sd) of observed values under their predictions: uniform on (0, 1)
    for a calibrated model"""
    u = (forward(y2, psi, kind, meta2) - np.asarray(zmean, np.float64)) / np.sqrt(np.asarray(zvar, np.float64))
    nd = NormalDist()
    return np.vectorize(nd.cdf, otypes=[np.float64])(u)
