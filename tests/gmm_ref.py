"""The definition medgp_gmm_fit is held to (numpy, fp64): EM for a full-covariance Gaussian mixture from a supplied start, the
restatement of scikit-learn's GaussianMixture(covariance_type='full') as the reference uses it (ref: medgpc/clustering/
cluster.py:23-46), and the reference's selection rule.  tests/test_clustering.py measures it against scikit-learn.

Start: hard labels -> one-hot responsibilities -> one M-step (an empty class is allowed: the 10 eps keeps its mean finite).
M-step: n_k = sum_i r_ik + 10 eps; w = n_k / n; mu_k = sum r_ik x_i / n_k; S_k = sum r_ik (x_i - mu_k)(x_i - mu_k)^T / n_k + reg I;
        L_k = chol(S_k) -- a pivot <= 0 or NaN fails the run.
E-step: log p_ik = -1/2 (d log 2pi + |L_k^-1 (x_i - mu_k)|^2) - sum log diag L_k + log w_k (the centred form: scikit-learn subtracts
        after the product); lse_i = logsumexp_k; r_ik = exp(log p_ik - lse_i); lb = mean lse.
Loop:   lb = -inf; it = 1 .. max_iter: E, M, change = lb - prev; converged when |change| < tol.
After:  one E-step: assign = first arg max, score = mean lse, bic = -2 score n + (K d (d + 1) / 2 + K d + K - 1) log n.
"""
import json
import os

import numpy as np
from scipy.linalg import solve_triangular

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gmm_spread.json")
KINDS = ("lower_bound", "bic", "weights", "means", "covs")


def _m_step(x, resp, reg_covar):
    """(nk, means, covs, chols) or None when a Cholesky pivot fails."""
    n, d = x.shape
    nk = resp.sum(axis=0) + 10.0 * np.finfo(np.float64).eps
    means = (resp.T @ x) / nk[:, None]
    K = resp.shape[1]
    covs = np.empty((K, d, d))
    chols = np.empty((K, d, d))
    for k in range(K):
        diff = x - means[k]
        covs[k] = (resp[:, k] * diff.T) @ diff / nk[k]
        covs[k].flat[:: d + 1] += reg_covar
        try:
            chols[k] = np.linalg.cholesky(covs[k])   # LAPACK potrf: raises on a pivot <= 0 or NaN
        except np.linalg.LinAlgError:
            return None
        if not np.all(np.isfinite(chols[k])):
            return None
    return nk, means, covs, chols


def _e_step(x, nk, means, chols):
    """(lse [n], resp [n, K])"""
    n, d = x.shape
    K = means.shape[0]
    logp = np.empty((n, K))
    for k in range(K):
        y = solve_triangular(chols[k], (x - means[k]).T, lower=True)
        logp[:, k] = -0.5 * (d * np.log(2.0 * np.pi) + np.sum(y * y, axis=0)) - np.sum(np.log(np.diag(chols[k]))) + np.log(nk[k] / n)
    m = logp.max(axis=1)
    lse = m + np.log(np.exp(logp - m[:, None]).sum(axis=1))
    return lse, np.exp(logp - lse[:, None])


def n_parameters(K, d):
    return K * d * (d + 1) // 2 + K * d + K - 1


def gmm_fit_one(x, K, label0, max_iter, tol, reg_covar=1e-6, trace=None):
    """One run.  Returns a dict: status (1 converged, 0 max_iter reached, -1 failed), n_iter, lower_bound, bic, weights [K],
    means [K, d], covs [K, d, d], assign [n], resp [n, K] (of the final E-step).  trace: a list that receives, per iteration,
    (change, largest condition number of the iteration's regularised covariances): the tests' conditions read it."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, d = x.shape
    label0 = np.asarray(label0)
    resp = np.zeros((n, K))
    resp[np.arange(n), label0] = 1.0
    failed = {"status": -1, "n_iter": 0, "lower_bound": np.nan, "bic": np.nan, "weights": np.full(K, np.nan),
              "means": np.full((K, d), np.nan), "covs": np.full((K, d, d), np.nan), "assign": np.full(n, -1, dtype=np.int32), "resp": None}
    par = _m_step(x, resp, reg_covar)
    if par is None:
        return failed
    lb, status, n_iter = -np.inf, 0, 0
    for it in range(1, max_iter + 1):
        prev = lb
        lse, resp = _e_step(x, par[0], par[1], par[3])
        par = _m_step(x, resp, reg_covar)
        n_iter = it
        if par is None:
            failed["n_iter"] = it
            return failed
        lb = lse.mean()
        change = lb - prev
        if trace is not None:
            trace.append((change, max(np.linalg.cond(c) for c in par[2])))
        if abs(change) < tol:
            status = 1
            break
    lse, resp = _e_step(x, par[0], par[1], par[3])
    score = lse.mean()
    return {"status": status, "n_iter": n_iter, "lower_bound": lb, "bic": -2.0 * score * n + n_parameters(K, d) * np.log(n),
            "weights": par[0] / n, "means": par[1], "covs": par[2], "assign": np.argmax(resp, axis=1).astype(np.int32), "resp": resp}


def gmm_fit(x, k, label0, max_iter=2000, tol=1e-3, reg_covar=1e-6, device=0, full=False):
    """The signature and return value of medgp_amd.capi.gmm_fit: (lower_bound, bic, n_iter, status) per run, with full=True also
    (weights [nruns, kmax], means [nruns, kmax, d], covs [nruns, kmax, d, d], assign [nruns, n], milliseconds)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    n, d = x.shape
    k = np.atleast_1d(np.asarray(k, dtype=np.int32))
    label0 = np.asarray(label0, dtype=np.int32).reshape(k.shape[0], n)
    nr, kmax = k.shape[0], int(k.max())
    lb, bic, nit, st = np.empty(nr), np.empty(nr), np.zeros(nr, np.int32), np.zeros(nr, np.int32)
    w, mu, cv, asg = np.zeros((nr, kmax)), np.zeros((nr, kmax, d)), np.zeros((nr, kmax, d, d)), np.zeros((nr, n), np.int32)
    for r in range(nr):
        o = gmm_fit_one(x, int(k[r]), label0[r], max_iter, tol, reg_covar)
        lb[r], bic[r], nit[r], st[r] = o["lower_bound"], o["bic"], o["n_iter"], o["status"]
        K = int(k[r])
        w[r, :K], mu[r, :K], cv[r, :K], asg[r] = o["weights"], o["means"], o["covs"], o["assign"]
    return (lb, bic, nit, st, w, mu, cv, asg, 0.0) if full else (lb, bic, nit, st)


def bound(kind):
    """B of the device parity bar B max(1, |ref|): 50 x the larger of the two recorded fp64 spreads of `kind` (definition against
    scikit-learn; definition against itself on permuted points).  50 is forecast_ref.lpd_bound's factor for a device summation
    order against numpy's."""
    rec = json.load(open(GOLDEN))
    return 50.0 * max(rec["vs_sklearn"][kind], rec["vs_permuted"][kind])


def rel_err(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - ref) / np.maximum(1.0, np.abs(ref))))


def sklearn_fit(x, K, label0, max_iter, tol, reg_covar=1e-6):
    """scikit-learn's own GaussianMixture.fit from the SAME start: a subclass whose only change is that the initial
    responsibilities are the one-hot label0 instead of a k-means result.  Returns gmm_fit_one's dict (without resp)."""
    import warnings
    from sklearn.mixture import GaussianMixture

    x = np.ascontiguousarray(x, dtype=np.float64)
    onehot = np.zeros((x.shape[0], K))
    onehot[np.arange(x.shape[0]), np.asarray(label0)] = 1.0

    class FromLabels(GaussianMixture):
        def _initialize_parameters(self, X, random_state):
            self._initialize(X, onehot)

    gm = FromLabels(n_components=K, covariance_type="full", max_iter=max_iter, n_init=1, tol=tol, reg_covar=reg_covar)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm.fit(x)
    return {"status": int(bool(gm.converged_)), "n_iter": int(gm.n_iter_), "lower_bound": float(gm.lower_bound_), "bic": float(gm.bic(x)),
            "weights": gm.weights_.copy(), "means": gm.means_.copy(), "covs": gm.covariances_.copy(),
            "assign": gm.predict(x).astype(np.int32)}
