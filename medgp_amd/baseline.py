"""Per-covariate baselines for the zero-mean GP: helpers around Context.mean_nlml_grad / Context.mean_posterior
(medgp_mean_nlml_grad, medgp_mean_posterior_batch).

The model is y = H beta + f + noise with one constant beta_d per covariate, either FIXED at given values (the reference's
c_meanfunc_constMO, whose mean hypers follow the covariance hypers: theta_ref = [lik | cov | mean]) or given the Gaussian prior
beta_d ~ N(b0_d, 1 / lam_d) and integrated out in closed form, which adds no hyper to optimise.  lam_d = 0 is the flat prior.
"""
import math

import numpy as np


def standard_prior(D):
    """(b0, lam) = (0, 1) per covariate: the natural prior for z-scored data"""
    return np.zeros(D), np.ones(D)


def flat(D, b0=None):
    """(b0, lam) of the flat prior (lam = 0: b0 does not matter; every covariate must then have an observation)"""
    return (np.zeros(D) if b0 is None else np.asarray(b0, np.float64).reshape(D)), np.zeros(D)


def fixed(m):
    """keyword arguments of Context.mean_nlml_grad / mean_posterior for the fixed mean m [D] or [nbatch, D]"""
    return dict(b0=np.asarray(m, np.float64), lam=None, fixed=True)


def prior_grad(beta, beta_cov, b0, lam):
    """(d nlml / d b0, d nlml / d log lam), each shaped like beta, of the marginalised objective from its outputs beta = beta^ and
    beta_cov = A^-1:  d/d b0_d = -lam_d (beta^_d - b0_d),  d/d lam_d = (A^-1)_dd / 2 + (beta^_d - b0_d)^2 / 2 - 1 / (2 lam_d).
    A flat covariate (lam_d = 0) has no parameter: both lines are 0."""
    beta, b0, lam = np.asarray(beta, np.float64), np.asarray(b0, np.float64), np.asarray(lam, np.float64)
    b0, lam = np.broadcast_to(b0, beta.shape), np.broadcast_to(lam, beta.shape)
    delta = beta - b0
    diag = np.diagonal(np.asarray(beta_cov, np.float64), axis1=-2, axis2=-1)
    pos = lam > 0
    return -(lam * delta), np.where(pos, lam * (diag / 2 + delta * delta / 2) - 0.5, 0.0)


def reference_theta(theta, m):
    """the reference's hyper vector [lik | cov | mean] from this library's theta [.., H] and the mean m [.., D]"""
    return np.concatenate([np.asarray(theta, np.float64), np.asarray(m, np.float64)], axis=-1)


def split_reference_theta(theta_ref, D):
    """(theta [.., H], m [.., D]) of a vector in the reference's layout"""
    theta_ref = np.asarray(theta_ref, np.float64)
    return theta_ref[..., :theta_ref.shape[-1] - D], theta_ref[..., theta_ref.shape[-1] - D:]


def split_reference_grad(grad, dmean):
    """the gradient in the reference's layout [lik | cov | mean] from grad [.., H] and dmean [.., D] of a FIXED call
    (ref: inference/c_inference_exact.cpp:221-232 appends the mean lines behind the covariance lines)"""
    return np.concatenate([np.asarray(grad, np.float64), np.asarray(dmean, np.float64)], axis=-1)


def objective(ctx, slots, b0, lam=None, fixed=False, reference_layout=False):
    """A closure x -> (values [nbatch], grads) for an optimiser.  Default: x = theta [nbatch, H], the baseline held at (b0, lam) or,
    fixed=True, at the mean b0; grads [nbatch, H].  reference_layout=True (fixed only): x = [theta | m] per patient in the reference's
    layout, the mean is optimised with the hypers and grads are [nbatch, H + D], as a caller ported from c_meanfunc_constMO expects."""
    slots = np.ascontiguousarray(slots, dtype=np.int32).ravel()
    nb = slots.shape[0]
    if reference_layout and not fixed:
        raise ValueError("reference_layout needs fixed=True: the marginalised baseline has no mean hypers")

    def f(x):
        x = np.asarray(x, np.float64).reshape(nb, -1)
        if reference_layout:
            th, m = split_reference_theta(x, x.shape[1] - ctx.H)
            r = ctx.mean_nlml_grad(slots, th, m, fixed=True)
            return r["nlml"], split_reference_grad(r["grad"], r["dmean"])
        r = ctx.mean_nlml_grad(slots, x, b0, lam, fixed=fixed)
        return r["nlml"], r["grad"]
    return f


def interval(mean, var, level=0.95):
    """(lo, hi) of the central prediction interval of a normal forecast"""
    p = 0.5 + level / 2.0
    z = 0.0
    for _ in range(60):   # the standard normal quantile by Newton steps on erf
        z -= (0.5 * (1.0 + math.erf(z / math.sqrt(2.0))) - p) / (math.exp(-z * z / 2) / math.sqrt(2 * math.pi))
    mean, s = np.asarray(mean, np.float64), np.sqrt(np.asarray(var, np.float64))
    return mean - z * s, mean + z * s
