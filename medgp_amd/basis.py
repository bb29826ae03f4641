"""Fixed effects for the GP: bases of trends and intervention effects for Context.set_basis / basis_nlml_grad / basis_posterior
(medgp_set_basis, medgp_basis_nlml_grad, medgp_basis_posterior_batch).  numpy only.

The model is y = H beta + f + noise with any H [n, p], p <= 64; beta is either fixed or given the prior beta_c ~ N(b0_c, 1 / lam_c) and
integrated out in closed form (lam_c = 0: flat).  A column is a function of (meta, t) -- the covariate and the time of a point -- so
the SAME recipe gives the rows of the observations (set_basis) and of the test points (basis_posterior's h2_list):

    design = Design([intercept(D), linear(D, origin=t.mean(), scale=t.std()), step(on=30.0, off=54.0, covariates=[2])])
    ctx.set_basis([0], [design.design(meta, t)])
    r = ctx.basis_nlml_grad([0], theta, *flat_prior(design.p))
    est, sd, z, prob = effect(r["beta"][0], r["beta_cov"][0], design.contrast("step[30,54)@2"))

A nearly dependent basis (uncentred time beside an intercept, a step that covers all observations of its covariate, two overlapping
ramps) makes A = Lambda + H^T K^-1 H ill-conditioned under small lam: centre and scale, and read `conditioning(H)` first.
"""
import math

import numpy as np

from .baseline import interval, prior_grad   # noqa: F401  (the same formulas with p in place of D)


class _Columns:
    """columns of a basis: names and a function (meta [n] int, t [n] float64) -> [n, k]"""

    def __init__(self, names, fn):
        self.names, self.fn = list(names), fn

    def __call__(self, meta, t):
        t = np.asarray(t, np.float64).ravel()
        meta = np.zeros(t.shape[0], np.int64) if meta is None else np.asarray(meta, np.int64).ravel()
        out = np.asarray(self.fn(meta, t), np.float64).reshape(t.shape[0], len(self.names))
        return out


def _mask(meta, covariates):
    return np.ones(meta.shape[0], bool) if covariates is None else np.isin(meta, np.asarray(list(covariates), np.int64))


def _tag(covariates):
    return "" if covariates is None else "@" + ",".join(str(int(c)) for c in covariates)


def intercept(D):
    """one constant per covariate: the indicator basis of the baseline calls"""
    return _Columns([f"intercept{d}" for d in range(D)], lambda m, t: (m[:, None] == np.arange(D)[None, :]).astype(np.float64))


def linear(D, origin, scale):
    """one slope per covariate in the centred and scaled time (t - origin) / scale, so that the column is O(1)"""
    origin, scale = float(origin), float(scale)
    if not scale > 0:
        raise ValueError("scale must be positive")
    return _Columns([f"slope{d}" for d in range(D)],
                    lambda m, t: (m[:, None] == np.arange(D)[None, :]) * ((t - origin) / scale)[:, None])


def step(on, off=math.inf, covariates=None):
    """1 while on <= t < off (a drug runs, a ventilator setting holds) on the listed covariates (None: all), else 0"""
    on, off = float(on), float(off)
    return _Columns([f"step[{on:g},{off:g}){_tag(covariates)}"], lambda m, t: ((t >= on) & (t < off) & _mask(m, covariates)).astype(np.float64))


def ramp(on, off, covariates=None):
    """0 before on, rising linearly to 1 at off, 1 afterwards"""
    on, off = float(on), float(off)
    if not off > on:
        raise ValueError("ramp needs off > on")
    return _Columns([f"ramp[{on:g},{off:g}]{_tag(covariates)}"], lambda m, t: np.clip((t - on) / (off - on), 0.0, 1.0) * _mask(m, covariates))


def harmonic(period, covariates=None):
    """cos and sin of 2 pi t / period (period = 24: time of day), shared by the listed covariates"""
    period = float(period)
    w = 2.0 * math.pi / period
    return _Columns([f"cos{period:g}{_tag(covariates)}", f"sin{period:g}{_tag(covariates)}"],
                    lambda m, t: np.stack([np.cos(w * t), np.sin(w * t)], axis=1) * _mask(m, covariates)[:, None])


def dose(times, amounts, covariates=None):
    """the amount of the dose in force at t: amounts[k] from times[k] until times[k + 1] (0 before the first), piecewise constant"""
    times, amounts = np.asarray(times, np.float64).ravel(), np.asarray(amounts, np.float64).ravel()
    if times.shape != amounts.shape or np.any(np.diff(times) <= 0):
        raise ValueError("dose: times strictly increasing, one amount per time")

    def fn(m, t):
        k = np.searchsorted(times, t, side="right") - 1
        return np.where(k >= 0, amounts[np.maximum(k, 0)], 0.0) * _mask(m, covariates)
    return _Columns([f"dose{_tag(covariates)}"], fn)


class Design:
    """a basis as a list of column builders: design(meta, t) -> H [n, p]; names label the columns"""

    def __init__(self, parts):
        self.parts = list(parts)
        self.names = [n for p in self.parts for n in p.names]
        self.p = len(self.names)
        if not 1 <= self.p <= 64:
            raise ValueError(f"a basis has 1 .. 64 columns, not {self.p}")

    def design(self, meta, t):
        return np.ascontiguousarray(np.concatenate([p(meta, t) for p in self.parts], axis=1))

    def contrast(self, name, weight=1.0):
        """the unit contrast [p] that picks the named column"""
        c = np.zeros(self.p)
        c[self.names.index(name)] = weight
        return c


def flat_prior(p):
    """(b0, lam) of the flat prior on every coefficient: the patient's rows must then determine them all"""
    return np.zeros(p), np.zeros(p)


def normal_prior(p, sd=1.0, b0=None):
    """(b0, lam) of beta_c ~ N(b0_c, sd^2)"""
    return (np.zeros(p) if b0 is None else np.asarray(b0, np.float64).reshape(p)), np.full(p, 1.0 / float(sd) ** 2)


def effect(beta, beta_cov, contrast):
    """(estimate, sd, z, prob_positive) of the linear combination contrast^T beta under its posterior N(beta, beta_cov)"""
    c = np.asarray(contrast, np.float64).ravel()
    est = float(c @ np.asarray(beta, np.float64).ravel())
    var = float(c @ np.asarray(beta_cov, np.float64) @ c)
    sd = math.sqrt(max(var, 0.0))
    if sd == 0.0:
        return est, 0.0, math.copysign(math.inf, est) if est else 0.0, 1.0 if est > 0 else 0.0
    z = est / sd
    return est, sd, z, 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))


def conditioning(H):
    """the condition number of H with every column scaled to unit length (zero columns left out; inf: dependent columns).  Large
    values (beyond ~1e4) mean coefficients that the data cannot tell apart under a flat prior."""
    H = np.asarray(H, np.float64)
    nrm = np.sqrt(np.sum(H * H, axis=0))
    Hn = H[:, nrm > 0] / nrm[nrm > 0]
    if Hn.shape[1] == 0:
        return math.inf
    s = np.linalg.svd(Hn, compute_uv=False)
    if Hn.shape[0] < Hn.shape[1] or s[-1] <= s[0] * Hn.shape[1] * np.finfo(np.float64).eps:
        return math.inf
    return float(s[0] / s[-1])


def objective(ctx, slots, b0, lam=None, fixed=False, with_coefficients=False):
    """A closure x -> (values [nbatch], grads) for an optimiser over the slots' resident bases.  Default: x = theta [nbatch, H], the
    coefficients held at the prior (b0, lam) or, fixed=True, at b0; grads [nbatch, H].  with_coefficients=True (fixed only):
    x = [theta | beta] per patient, the coefficients are optimised with the hypers and grads are [nbatch, H + p]."""
    slots = np.ascontiguousarray(slots, dtype=np.int32).ravel()
    nb = slots.shape[0]
    if with_coefficients and not fixed:
        raise ValueError("with_coefficients needs fixed=True: marginalised coefficients are not parameters")

    def f(x):
        x = np.asarray(x, np.float64).reshape(nb, -1)
        if with_coefficients:
            r = ctx.basis_nlml_grad(slots, x[:, :ctx.H], x[:, ctx.H:], fixed=True)
            return r["nlml"], np.concatenate([r["grad"], r["dbeta"]], axis=1)
        r = ctx.basis_nlml_grad(slots, x, b0, lam, fixed=fixed)
        return r["nlml"], r["grad"]
    return f
