"""numpy reference of medgp_forecast_batch: point j predicted from the first prefix[j] observations of the patient.

refit() IS the definition: for every distinct prefix p the restatement of GP_Regression::predict (posterior_ref.restate, on the
oracle's Gram matrix) applied to the training set obs[0:p]; p = 0 is the prior.  With jitter_rounds = k the k extra
diag(sigma^2) go on the prefix block.  lpd = -1/2 log(2 pi var) - 1/2 (y2 - mean)^2 / var from that fp64 mean / var.

one_factor() is the identity the device uses: ONE factor L of the whole patient, V = L^-1 K*, z = L^-1 y, and the sums of
column j stopped at row prefix[j].  test_forecast.py holds the two together on every input of the GPU tests and records their
spread in lpd (tests/golden/forecast_lpd_spread.json), from which the GPU test's lpd bound is taken (lpd_bound)."""
import json
import os

import numpy as np

from oracle import oracle as O
import posterior_ref as PR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forecast_lpd_spread.json")
LPD_FACTOR = 50.0     # the device's summation order against numpy's on the same fp64 problem
LPD_FLOOR = 1e-12


def log_density(y2, mean, var, pi=O.REF_PI):
    y2 = np.asarray(y2, np.float32).astype(np.float64)
    return -0.5 * np.log(2.0 * pi * var) - 0.5 * (y2 - mean) ** 2 / var


def _prior(kidx, Q, D, R, theta, meta2, t2):
    """(mean, var) without any observation: 0 and the Gram diagonal of the test points (k** + sigma^2)"""
    multi = kidx == O.KERNEL_LMC_SM
    K = O.gram(kidx, Q, D, R, np.asarray(meta2, np.int32) if multi else None, np.asarray(t2, np.float32), theta)
    return np.zeros(K.shape[0]), np.diag(K).copy()


def refit(kidx, Q, D, R, meta, t, y, theta, meta2, t2, prefix, y2=None, jitter_rounds=0, pi=O.REF_PI):
    """Returns (mean[m], var[m], lpd[m] or None) in fp64.  meta / meta2 are ignored for SE / SM (may be None)."""
    multi = kidx == O.KERNEL_LMC_SM
    t2 = np.asarray(t2, np.float32)
    m = t2.shape[0]
    meta2 = np.asarray(meta2, np.int32) if multi else np.zeros(m, np.int32)
    prefix = np.asarray(prefix, np.int64)
    assert prefix.shape == (m,) and (m == 0 or (prefix.min() >= 0 and prefix.max() <= np.shape(t)[0]))
    mean, var = np.zeros(m), np.zeros(m)
    for p in np.unique(prefix):
        sel = np.flatnonzero(prefix == p)
        if p == 0:
            mean[sel], var[sel] = _prior(kidx, Q, D, R, theta, meta2[sel], t2[sel])
            continue
        mean[sel], var[sel], _ = PR.restate(kidx, Q, D, R, meta[:p] if multi else None, t[:p], y[:p], theta,
                                            meta2[sel] if multi else None, t2[sel], jitter_rounds)
    return mean, var, (None if y2 is None else log_density(y2, mean, var, pi))


def one_factor(kidx, Q, D, R, meta, t, y, theta, meta2, t2, prefix, y2=None, jitter_rounds=0, pi=O.REF_PI):
    """The same outputs from one factor of the whole patient (rows < p of solve(L, K*))."""
    multi = kidx == O.KERNEL_LMC_SM
    t2 = np.asarray(t2, np.float32)
    m, n = t2.shape[0], np.shape(t)[0]
    meta2 = np.asarray(meta2, np.int32) if multi else np.zeros(m, np.int32)
    prefix = np.asarray(prefix, np.int64)
    if n == 0:
        mean, var = _prior(kidx, Q, D, R, theta, meta2, t2)
    else:
        Ks, _, Lc, kss, sig2_2, _ = PR.terms(kidx, Q, D, R, meta, t, y, theta, meta2 if multi else None, t2, jitter_rounds)
        V = np.linalg.solve(Lc, Ks)
        z = np.linalg.solve(Lc, np.asarray(y, np.float32).astype(np.float64))
        keep = np.arange(n)[:, None] < prefix[None, :]
        Vm = np.where(keep, V, 0.0)
        mean = Vm.T @ z
        var = kss - np.sum(Vm * Vm, axis=0) + sig2_2
    return mean, var, (None if y2 is None else log_density(y2, mean, var, pi))


def cond(kidx, Q, D, R, meta, t, theta):
    multi = kidx == O.KERNEL_LMC_SM
    w = np.linalg.eigvalsh(O.gram(kidx, Q, D, R, np.asarray(meta, np.int32) if multi else None, np.asarray(t, np.float32), theta))
    return float(w[-1] / w[0])


def lpd_error(dev, ref):
    """largest |dev - ref| / max(1, |ref|); NaN counts as infinite"""
    ref = np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    e = np.abs(np.asarray(dev, np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    return float(np.where(np.isnan(e), np.inf, e).max())


def lpd_bound():
    """B of |dev - ref| <= B max(1, |ref|): LPD_FACTOR x the recorded spread of the two fp64 restatements, not below LPD_FLOOR"""
    return max(LPD_FACTOR * float(json.load(open(GOLDEN))["lpd_spread"]), LPD_FLOOR)


def check_forecast(kidx, D, theta, meta2, prefix, ref, out):
    """One patient's device output (mean, var, lpd or None) against ref = refit(...): mean / var to the project's bar (two fp32
    ulps of max(|ref|, 1e-3 S)), var >= sigma^2_{meta2}, prefix 0 has mean exactly 0.0f, lpd within lpd_bound().
    Returns (mean error in fp32 ulps, var error in fp32 ulps, lpd error)."""
    rm, rv, rl = ref
    mean, var, lpd = out
    m = rm.shape[0]
    assert mean.shape == (m,) and var.shape == (m,) and mean.dtype == np.float32 and var.dtype == np.float32
    if m == 0:
        return 0.0, 0.0, 0.0
    PR.check_posterior(kidx, D, theta, meta2, (rm, rv, None), mean, var)
    zero = np.asarray(prefix) == 0
    assert np.all(mean[zero] == 0.0) and not np.any(np.signbit(mean[zero])), "prefix 0: the mean is not exactly 0.0f"
    el = 0.0
    if rl is not None:
        assert lpd is not None and lpd.shape == (m,) and lpd.dtype == np.float64
        el = lpd_error(lpd, rl)
        assert el <= lpd_bound(), f"lpd: {el:.3g} relative, bound {lpd_bound():.3g}"
    # (an all-prior patient has reference means of exactly 0: no scale, and the equality above is the check)
    return (PR.ulp_error(mean, rm) if np.any(rm != 0) else 0.0), PR.ulp_error(var, rv), el
