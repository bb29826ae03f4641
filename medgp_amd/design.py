"""What to measure next, from the joint posterior of linear functionals (Context.functionals_joint / medgp_functional_joint_batch).
Pure numpy in float64; the device supplies the covariance.

Put the TARGETS (window means, changes, points -- medgp_amd.functionals) and the CANDIDATE measurements (single-term `point`
functionals, `candidates`) into ONE list of functionals of a patient; `cov` below is that patient's fcov [F, F] and targets / cands
are index lists into it.  A measurement of candidate c = (m, t) observes f_m(t) + noise of variance noise_c, and conditioning a
Gaussian on it lowers every covariance by a rank-1 term that does not depend on the value measured:
    cov'[i, j] = cov[i, j] - cov[i, c] cov[c, j] / (cov[c, c] + noise_c)
so the expected drop of a target's variance is cov[t, c]^2 / (cov[c, c] + noise_c), known before the measurement is taken.

fcov is LATENT (no sigma^2): the noise of the future measurement is the caller's `noise` (`noise_variance` gives the model's sigma^2
of a covariate).  After k jitter rounds (status[b] = k > 0) fcov is the posterior covariance under K + k diag(sigma^2), the matrix
that was factored -- the past measurements then count as noisier than the model says; the new measurement's own noise is still
whatever the caller passes."""
import numpy as np

from . import functionals
from .capi import KERNEL_LMC_SM


def noise_variance(kernel_index, D, theta, meta):
    """sigma^2 of the covariates `meta` (int array, ignored for SE / SM) under the hyper-parameters theta of ONE patient: the likelihood
    hypers theta[:D] (SE / SM: theta[0]) are log sigma.  This is the model's noise of one measurement, after any number of jitter
    rounds: those change the matrix that was factored, not the likelihood."""
    theta = np.asarray(theta, np.float64).ravel()
    meta = np.asarray(meta, np.int64).ravel()
    if kernel_index != KERNEL_LMC_SM:
        return np.full(meta.shape[0], np.exp(2.0 * theta[0]))
    if meta.size and (meta.min() < 0 or meta.max() >= D):
        raise ValueError(f"meta outside [0, {D})")
    return np.exp(2.0 * theta[:D])[meta]


def candidates(covariates, times):
    """the measurement grid covariates x times as a list of functionals.point, covariate-major: candidate i * len(times) + j is
    (covariates[i], times[j])"""
    return [functionals.point(int(m), float(t)) for m in np.asarray(covariates).ravel() for t in np.asarray(times).ravel()]


def _check(cov, idx_lists, noise, cands):
    cov = np.asarray(cov, np.float64)
    if cov.ndim != 2 or cov.shape[0] != cov.shape[1]:
        raise ValueError(f"cov has shape {cov.shape}, expected (F, F)")
    out = []
    for name, idx in idx_lists:
        idx = np.asarray(idx, np.int64)
        if idx.ndim != 1:
            raise ValueError(f"{name} has shape {idx.shape}, expected a list of indices")
        if idx.size and (idx.min() < 0 or idx.max() >= cov.shape[0]):
            raise ValueError(f"{name} outside [0, {cov.shape[0]})")
        out.append(idx)
    noise = np.asarray(noise, np.float64)
    if noise.shape != out[cands].shape:
        raise ValueError(f"noise has shape {noise.shape} for {out[cands].shape[0]} measurements")
    return [cov] + out + [noise]


def variance_reduction(cov, targets, cands, noise):
    """[n_t, n_c]: the expected drop cov[t, c]^2 / (cov[c, c] + noise_c) of the posterior variance of target t from ONE measurement of
    candidate c (noise [n_c]: its noise variance).  NaN where the denominator is <= 0 (a candidate the data already determine, measured
    without noise: nothing to divide by), never infinity.  A failed patient's NaN covariance gives NaN."""
    cov, targets, cands, noise = _check(cov, (("targets", targets), ("cands", cands)), noise, 1)
    den = cov[cands, cands] + noise
    ok = den > 0
    return np.where(ok[None, :], cov[np.ix_(targets, cands)] ** 2 / np.where(ok, den, 1.0)[None, :], np.nan)


def _downdate(cov, c, noise_c):
    den = cov[c, c] + noise_c
    if not den > 0:
        raise ValueError(f"measurement {c}: cov[c, c] + noise = {den} is not positive")
    col = cov[:, c].copy()
    return cov - np.outer(col, col) / den


def condition(cov, picks, noise):
    """The covariance [F, F] after measuring the functionals `picks` (indices into cov, usually candidates; noise [len(picks)]), one
    after another by rank-1 downdates.  No measured values are needed: the variance does not depend on them.  The same index may be
    measured twice (a repeated measurement).  Raises where cov[c, c] + noise_c <= 0 at its turn."""
    cov, picks, noise = _check(cov, (("picks", picks),), noise, 0)
    for c, s in zip(picks, noise):
        cov = _downdate(cov, int(c), float(s))
    return cov


def greedy(cov, targets, cands, noise, k, weights=None):
    """k measurements chosen one at a time: each pick is the candidate, among those not picked yet, whose measurement lowers
    sum_t weights[t] var(target t) most (weights None: all 1), and the covariance is downdated before the next pick.  Returns
    (picks [k] as positions in `cands`, sums [k]: the weighted sum of the target variances after every pick).  Candidates whose
    denominator is <= 0 are never picked; raises if fewer than k candidates can be."""
    cov, targets, cands, noise = _check(cov, (("targets", targets), ("cands", cands)), noise, 1)
    w = np.ones(targets.shape[0]) if weights is None else np.asarray(weights, np.float64)
    if w.shape != targets.shape:
        raise ValueError(f"weights has shape {w.shape} for {targets.shape[0]} targets")
    k = int(k)
    if k < 0 or k > cands.shape[0]:
        raise ValueError(f"k = {k} picks from {cands.shape[0]} candidates")
    free = np.ones(cands.shape[0], bool)
    picks, sums = [], []
    for _ in range(k):
        gain = np.where(free, w @ variance_reduction(cov, targets, cands, noise), np.nan)
        if np.all(np.isnan(gain)):
            raise ValueError(f"only {len(picks)} of {k} picks possible: no candidate with cov[c, c] + noise > 0 is left")
        j = int(np.nanargmax(gain))
        cov = _downdate(cov, int(cands[j]), float(noise[j]))
        free[j] = False
        picks.append(j)
        sums.append(float(w @ cov[targets, targets]))
    return np.array(picks, np.int64), np.array(sums, np.float64)
