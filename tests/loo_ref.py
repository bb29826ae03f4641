"""numpy restatement of the leave-one-out / leave-group-out predictive distribution of a patient's own observations
(medgp_loo_batch), on the oracle's Gram matrix.  The reference has no such function: refit() IS the definition -- for every
group drop its rows and columns, factor the rest, take the Gaussian conditional of the group:
    mean_B = K_Br K_rr^-1 y_r,   cov_B = K_BB - K_Br K_rr^-1 K_rB,   lpd_B = log N(y_B; mean_B, cov_B)
(an empty rest gives the prior: mean 0, cov K_BB).  via_inverse() is the identity the device uses (M = (K^-1)_BB,
cov_B = M^-1, mean_B = y_B - M^-1 alpha_B); test_loo.py holds the two together on every input of the GPU tests, so the bar
cannot be met or missed by the choice of reference.

check_loo() holds device output to the project's bars: mean / var within posterior_ref.FP32_BOUND = 2 fp32 ulps of
max(|ref|, 1e-3 S), lpd / total within nlml_truth.NLML_BUDGET_CAP = 1e-10 of max(1, |ref|).  The bars need K well conditioned
(cond(K) <= posterior_joint_ref.COND_MAX; cond(M) <= cond(K) by interlacing): a condition on the INPUTS, asserted in
test_loo.py for every case."""
import numpy as np

from oracle import oracle as O
from posterior_ref import FLOOR, FP32_BOUND, noise_var

LPD_BOUND = 1e-10   # nlml_truth.NLML_BUDGET_CAP: the project's nlml contract


def gram(kidx, Q, D, R, meta, t, theta, jitter_rounds=0):
    """K + jitter_rounds * diag(sigma^2): what the reference's retry loop factors after that many extra noise additions"""
    t = np.asarray(t, np.float32)
    n = t.shape[0]
    multi = kidx == O.KERNEL_LMC_SM
    meta = np.asarray(meta, np.int32) if multi else np.zeros(n, np.int32)
    K = O.gram(kidx, Q, D, R, meta if multi else None, t, theta).copy()
    if jitter_rounds:
        K[np.diag_indices(n)] += jitter_rounds * noise_var(kidx, D, theta, meta)
    return K


def _groups(n, group, ngroups):
    """(ids [n], G): None = every observation its own group"""
    if group is None:
        return np.arange(n), n
    group = np.asarray(group, np.int64)
    assert group.shape == (n,) and (n == 0 or (group.min() >= -1 and group.max() < ngroups))
    return group, int(ngroups)


def _gauss_logpdf(r, C, pi):
    Lc = np.linalg.cholesky(C)
    w = np.linalg.solve(Lc, r)
    return -0.5 * float(w @ w) - float(np.log(np.diag(Lc)).sum()) - 0.5 * r.shape[0] * np.log(2.0 * pi)


def refit(kidx, Q, D, R, meta, t, y, theta, group=None, ngroups=None, jitter_rounds=0, pi=O.REF_PI):
    """The definition.  Returns (mean[n], var[n], lpd[G], total) in fp64; mean / var are NaN where group is -1, lpd is 0.0
    for an empty group."""
    K = gram(kidx, Q, D, R, meta, t, theta, jitter_rounds)
    n = K.shape[0]
    yy = np.asarray(y, np.float32).astype(np.float64)
    ids, G = _groups(n, group, ngroups)
    mean, var, lpd = np.full(n, np.nan), np.full(n, np.nan), np.zeros(G)
    for gid in range(G):
        B = np.flatnonzero(ids == gid)
        if B.size == 0:
            continue
        rest = np.flatnonzero(ids != gid)
        if rest.size:
            Lr = np.linalg.cholesky(K[np.ix_(rest, rest)])
            A = np.linalg.solve(Lr, K[np.ix_(rest, B)])
            mu = A.T @ np.linalg.solve(Lr, yy[rest])
            Cb = K[np.ix_(B, B)] - A.T @ A
            Cb = 0.5 * (Cb + Cb.T)
        else:
            mu, Cb = np.zeros(B.size), K[np.ix_(B, B)]
        mean[B], var[B] = mu, np.diag(Cb)
        lpd[gid] = _gauss_logpdf(yy[B] - mu, Cb, pi)
    return mean, var, lpd, float(lpd.sum())


def via_inverse(kidx, Q, D, R, meta, t, y, theta, group=None, ngroups=None, jitter_rounds=0, pi=O.REF_PI):
    """The same outputs through one inverse: M = (K^-1)_BB, cov = M^-1, mean = y_B - M^-1 alpha_B,
    lpd = -1/2 alpha_B^T M^-1 alpha_B + 1/2 log det M - |B|/2 log 2 pi."""
    K = gram(kidx, Q, D, R, meta, t, theta, jitter_rounds)
    n = K.shape[0]
    yy = np.asarray(y, np.float32).astype(np.float64)
    ids, G = _groups(n, group, ngroups)
    Li = np.linalg.solve(np.linalg.cholesky(K), np.eye(n))
    Kinv = Li.T @ Li
    alpha = Kinv @ yy
    mean, var, lpd = np.full(n, np.nan), np.full(n, np.nan), np.zeros(G)
    for gid in range(G):
        B = np.flatnonzero(ids == gid)
        if B.size == 0:
            continue
        M = Kinv[np.ix_(B, B)]
        Rm = np.linalg.cholesky(0.5 * (M + M.T))
        w = np.linalg.solve(Rm, alpha[B])
        Ri = np.linalg.solve(Rm, np.eye(B.size))
        mean[B] = yy[B] - np.linalg.solve(Rm.T, w)
        var[B] = np.sum(Ri * Ri, axis=0)
        lpd[gid] = -0.5 * float(w @ w) + float(np.log(np.diag(Rm)).sum()) - 0.5 * B.size * np.log(2.0 * pi)
    return mean, var, lpd, float(lpd.sum())


def cond(K):
    w = np.linalg.eigvalsh(K)
    return float(w[-1] / w[0])


def errors(ref, y, out):
    """(mean error in fp32 ulps of max(|ref|, 1e-3 S), the same for var, largest lpd / total error relative to max(1, |ref|))
    of out = (mean, var, lpd, total) against ref; S as in check_loo.  NaN where the reference is NaN does not count; anywhere
    else it is infinite."""
    rm, rv, rl, rt = ref
    mean, var, lpd, total = out
    held = ~np.isnan(rm)
    yy = np.abs(np.asarray(y, np.float32).astype(np.float64))

    def ulps(dev, r, S):
        if not held.any():
            return 0.0
        e = np.abs(np.asarray(dev, np.float64)[held] - r[held]) / (2.0 ** -23 * np.maximum(np.abs(r[held]), FLOOR * S))
        return float(np.where(np.isnan(e), np.inf, e).max())

    Sm = max(np.abs(rm[held]).max(), yy.max()) if held.any() else 1.0
    Sv = rv[held].max() if held.any() else 1.0
    el = np.abs(np.append(np.asarray(lpd, np.float64), total) - np.append(rl, rt)) / np.maximum(1.0, np.abs(np.append(rl, rt)))
    return ulps(mean, rm, Sm), ulps(var, rv, Sv), float(np.where(np.isnan(el), np.inf, el).max())


def check_loo(ref, y, out, scale=1.0):
    """One patient's output (mean, var, lpd, total) against ref = refit(...).  mean and var within two fp32 ulps of
    max(|ref|, 1e-3 S): S for var the patient's largest reference var, S for mean the patient's largest of |ref mean| and |y|
    (the mean is a difference from y; with one all-inclusive group the reference mean is exactly 0).  lpd and total within
    1e-10 max(1, |ref|).  var > 0; an observation never held out has NaN mean and var.  scale < 1 tightens every bar (the CPU
    comparison of the two restatements uses 1/8).  Returns errors(...)."""
    rm, rv, rl, rt = ref
    mean, var, lpd, total = out
    assert np.shape(mean) == rm.shape and np.shape(var) == rv.shape and np.shape(lpd) == rl.shape, (np.shape(mean), np.shape(lpd), rm.shape, rl.shape)
    out_of = np.isnan(rm)
    assert np.all(np.isnan(np.asarray(mean)[out_of])) and np.all(np.isnan(np.asarray(var)[out_of])), "an observation never held out has a mean / var"
    assert np.all(np.asarray(var)[~out_of] > 0), "var <= 0 (or NaN)"
    em, ev, el = errors(ref, y, out)
    # FP32_BOUND is 2 ulps (2^-22 = 2 x 2^-23)
    assert em <= scale * FP32_BOUND * 2.0 ** 23, f"mean: {em:.3g} fp32 ulps"
    assert ev <= scale * FP32_BOUND * 2.0 ** 23, f"var: {ev:.3g} fp32 ulps"
    assert el <= scale * LPD_BOUND, f"lpd / total: {el:.3g} relative"
    return em, ev, el
