"""What the slope posterior of Context.trend / medgp_trend_batch says about a patient (pure numpy; the posterior itself comes
from the device): the probability that a covariate is rising at t, an interval for its rate of change, and the grid of test
points over a patient's record.

The latent slope f'(t*) given the data is Gaussian with mean dmean and variance dvar (include/medgp_hip.h), so
    P(f'(t*) > 0) = Phi(dmean / sqrt(dvar)),      f'(t*) in dmean +- z_level sqrt(dvar).
"""
import math
from statistics import NormalDist

import numpy as np

_erfc = np.frompyfunc(math.erfc, 1, 1)


def prob_rising(dmean, dvar):
    """Phi(dmean / sqrt(dvar)): the posterior probability that the latent function is increasing at the point.  dvar == 0 (a
    slope known exactly) gives 0, 1/2 or 1 by the sign of dmean; NaN inputs (a failed patient) and dvar < 0 give NaN."""
    dm = np.asarray(dmean, np.float64)
    dv = np.asarray(dvar, np.float64)
    if dm.shape != dv.shape:
        raise ValueError(f"dmean has shape {dm.shape}, dvar {dv.shape}")
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(dv > 0, dm / np.sqrt(np.where(dv > 0, dv, 1.0)), np.nan)
    exact = (dv == 0) & ~np.isnan(dm)
    u = np.where(exact, np.where(dm > 0, np.inf, np.where(dm < 0, -np.inf, 0.0)), u)
    p = 0.5 * np.asarray(_erfc(-u / math.sqrt(2.0)), np.float64)   # erfc: no cancellation in the lower tail
    return p.reshape(dm.shape)


def rate_interval(dmean, dvar, level=0.95):
    """(lo, hi) of the central `level` interval of the slope, per hour in the units of y: dmean -+ z sqrt(dvar) with
    z = Phi^-1((1 + level) / 2) (1.96 for 95 %)."""
    if not 0.0 < level < 1.0:
        raise ValueError(f"level = {level} outside (0, 1)")
    dm = np.asarray(dmean, np.float64)
    dv = np.asarray(dvar, np.float64)
    if dm.shape != dv.shape:
        raise ValueError(f"dmean has shape {dm.shape}, dvar {dv.shape}")
    z = NormalDist().inv_cdf(0.5 * (1.0 + level))
    with np.errstate(invalid="ignore"):
        h = z * np.sqrt(dv)   # (dvar < 0 or NaN: NaN)
    return dm - h, dm + h


def grid(t, D, step_h):
    """Test points of every covariate on a time grid over ONE patient's record: times t_min, t_min + step_h, ... up to t_max
    (t_max itself is added when the last step falls short of it), repeated for the covariates 0 .. D - 1, covariate-major.
    Returns (meta2 int32[D * G], t2 float32[D * G]); an empty record gives empty arrays."""
    t = np.asarray(t, np.float64).ravel()
    D = int(D)
    if D < 1:
        raise ValueError(f"D = {D}")
    if not (step_h > 0 and math.isfinite(step_h)):
        raise ValueError(f"step_h = {step_h} must be finite and > 0")
    if t.shape[0] == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.float32)
    if not np.all(np.isfinite(t)):
        raise ValueError("non-finite time stamp")
    lo, hi = float(t.min()), float(t.max())
    g = lo + step_h * np.arange(int(math.floor((hi - lo) / step_h)) + 1)
    if g[-1] < hi:
        g = np.append(g, hi)
    return np.repeat(np.arange(D, dtype=np.int32), g.shape[0]), np.tile(g.astype(np.float32), D)
