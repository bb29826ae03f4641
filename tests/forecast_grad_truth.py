"""Extended-precision truth of medgp_forecast_grad: the negative h-hours-ahead forecast score and its gradient in the hyper
vector, built on nlml_truth's hyper transforms, Gram matrix, column Cholesky and triangular inverse and on loo_grad_truth's
W -> gradient lines.  The reference has no such output: this restatement IS the definition.

Observations in the caller's order; K = gram + noise (+ jitter_rounds diag(sigma^2)); scored observation i has a history length
p = prefix[i] in [0, i] (prefix[i] = -1: not scored):

    a_i = K[0:p,0:p]^-1 K[0:p,i]      mean_i = a_i^T y[0:p]      var_i = K[i,i] - K[0:p,i]^T a_i      r_i = y_i - mean_i
    lpd_i = -1/2 log(2 PI var_i) - 1/2 r_i^2 / var_i            J = - sum_{i scored} lpd_i
    u_i = [-a_i on [0,p) | 1 at i | 0 elsewhere]                 beta_i = [K[0:p,0:p]^-1 y[0:p] on [0,p) | 0 elsewhere]
    dJ / d theta_h = 1/2 tr(W_fc dK / d theta_h),   W_fc = sum_i [ g_i u_i u_i^T - e_i (beta_i u_i^T + u_i beta_i^T) ],
    g_i = (1 - r_i^2 / var_i) / var_i,   e_i = r_i / var_i

forecast_grad() is the definition BY REFIT: every distinct history length gets its own factorisation of its own leading block (the
same code in any dtype: program (a) in long double, program (b) in float64).  one_factor() is program (c): the identities the
device uses, in float64 on numpy's Cholesky of the whole K -- var_i and r_i from the band [p_i, i] of row i of L, T = U Mbar,
beta from running sums of U diag(z), W_fc = T Qm^T + Qm T^T.  PI = nlml_truth.REF_PI, no prior, any n >= 1.

The module also holds the cases shared by tests/test_forecast_grad.py (CPU: the budget conditions) and
tests/test_forecast_grad_gpu.py (the device held to the budget) and the budget constants, which are loo_grad_truth's.
"""
import numpy as np

import loo_grad_truth as G
import nlml_truth as T
from loo_grad_truth import COND_MAX, M_GRAD, M_OBJ, NAIVE_MAX_N, grad_from_w   # noqa: F401  (the budget rule is loo_grad_truth's)
from nlml_truth import GRAD_BUDGET_CAP, NLML_BUDGET_CAP, U64, budget, error_pair, spread   # noqa: F401

HORIZONS = [0.0, 6.0]      # hours


def _check_prefix(prefix, n):
    p = np.arange(n, dtype=np.int64) if prefix is None else np.asarray(prefix, np.int64).ravel()
    assert p.shape == (n,) and np.all(p >= -1) and np.all(p <= np.arange(n)), "prefix[i] must be -1 or in [0, i]"
    return p


def _w_fc(Um, Bm, g, e):
    W = (Um * g[None, :]) @ Um.T - (Bm * e[None, :]) @ Um.T - Um @ (Bm * e[None, :]).T
    return (W + W.T) / 2


def forecast_grad(kidx, Q, D, R, meta, t, y, theta, prefix=None, dtype=np.longdouble, jitter_rounds=0, want_grad=True, form=None,
                  want_parts=False):
    """(J, grad[H] or None) in precision dtype by refit of every distinct history length.  want_parts: also (lpd[n] with 0 where
    not scored, W_fc or None).  form: as loo_grad_truth.loo_grad."""
    X = dtype
    t32 = np.asarray(t, np.float32)
    n = t32.shape[0]
    assert n >= 1
    if form is None:
        form = "naive" if n <= NAIVE_MAX_N else "blocks"
    pf = _check_prefix(prefix, n)
    yy = np.asarray(y, np.float32).astype(X)
    K = T.gram(kidx, Q, D, R, meta, t32, theta, X, jitter_rounds)
    log2pi = np.log(2 * T.transform(kidx, Q, D, R, theta, X)["pi"])
    scored = np.flatnonzero(pf >= 0)
    lpd = np.zeros(n, X)
    Um, Bm = np.zeros((n, scored.shape[0]), X), np.zeros((n, scored.shape[0]), X)
    g, e = np.zeros(scored.shape[0], X), np.zeros(scored.shape[0], X)
    col = {int(i): c for c, i in enumerate(scored)}
    for p in np.unique(pf[scored]):
        p = int(p)
        if p > 0:
            Li = T._tri_inverse(T._chol_columns(K[:p, :p]))
            beta = Li.T @ (Li @ yy[:p])
        for i in np.flatnonzero(pf == p):
            i = int(i)
            c = col[i]
            Um[i, c] = 1
            if p > 0:
                a = Li.T @ (Li @ K[:p, i])
                Um[:p, c] = -a
                Bm[:p, c] = beta
                mean, var = a @ yy[:p], K[i, i] - K[:p, i] @ a
            else:
                mean, var = X(0), K[i, i]
            r = yy[i] - mean
            lpd[i] = -(log2pi + np.log(var)) / 2 - r * r / var / 2
            g[c] = (1 - r * r / var) / var
            e[c] = r / var
    J = -np.sum(lpd)
    W = _w_fc(Um, Bm, g, e) if want_grad or want_parts else None
    grad = grad_from_w(kidx, Q, D, R, meta, t32, theta, W, X, form) if want_grad else None
    return (J, grad, lpd, W) if want_parts else (J, grad)


def one_factor(kidx, Q, D, R, meta, t, y, theta, prefix=None, jitter_rounds=0, want_parts=False):
    """program (c): float64, ONE numpy Cholesky of the whole K and the device's identities; the gradient in block-sum form"""
    t32 = np.asarray(t, np.float32)
    n = t32.shape[0]
    pf = _check_prefix(prefix, n)
    yy = np.asarray(y, np.float32).astype(np.float64)
    K = T.gram(kidx, Q, D, R, meta, t32, theta, np.float64, jitter_rounds)
    L = np.linalg.cholesky(K)
    U = np.triu(np.linalg.inv(L).T)
    z = np.linalg.solve(L, yy)
    k = np.arange(n)
    sc = pf >= 0
    band = sc[:, None] & (k[None, :] >= pf[:, None]) & (k[None, :] <= k[:, None])      # [i, k]
    Mb = np.where(band, L, 0.0)
    var = np.sum(Mb * Mb, axis=1)
    r = Mb @ z
    with np.errstate(divide="ignore", invalid="ignore"):
        lpd = np.where(sc, -(np.log(2 * T.REF_PI) + np.log(var)) / 2 - r * r / var / 2, 0.0)
        g = np.where(sc, (1 - r * r / var) / var, 0.0)
        e = np.where(sc, r / var, 0.0)
    J = -np.sum(lpd)
    Tm = U @ Mb.T                                                                         # column i = u_i
    run = np.concatenate([np.zeros((n, 1)), np.cumsum(U * z[None, :], axis=1)], axis=1)   # run[j, p] = sum_{k < p} U[j,k] z[k]
    Bm = np.where(sc[None, :] & (k[:, None] < pf[None, :]), run[:, np.maximum(pf, 0)], 0.0) * e[None, :]
    Qm = Tm * (g / 2)[None, :] - Bm
    W = Tm @ Qm.T + Qm @ Tm.T
    W = (W + W.T) / 2
    grad = grad_from_w(kidx, Q, D, R, meta, t32, theta, W, np.float64, "blocks")
    return (J, grad, lpd, W) if want_parts else (J, grad)


def cond(kidx, Q, D, R, meta, t, theta, jitter_rounds=0):
    return G.cond(kidx, Q, D, R, meta, t, theta, jitter_rounds)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# The patients of loo_grad_truth._SPECS without the n = 512 one, each stably sorted by time -- so that its covariates interleave, the
# order a forecast is about -- at the horizons 0 h (everything strictly earlier) and 6 h.  Sizes as there: n = 1, 3, the 64-block edges
# 63 | 64 | 65, three blocks (130) and four (200); at 0 h the band of a row is a few columns inside one block or across a block edge, at
# 6 h of 200 h it spans blocks.
CASE_IDS = [c for c in G.CASE_IDS if c != "lmc_D24_n512"]
_CASES = {}


def case(cid):
    """loo_grad_truth.case(cid) with every patient stably sorted by time"""
    if cid not in _CASES:
        c = G.case(cid)
        pts = []
        for m, t, y in c["pts"]:
            o = np.argsort(t, kind="stable")
            pts.append((None if m is None else m[o], t[o], y[o]))
        _CASES[cid] = dict(c, pts=pts)
    return _CASES[cid]


fam = G.fam


def prefix_of(c, p, horizon):
    from medgp_amd.forecast import training_prefix
    return training_prefix(c["pts"][p][1], horizon)


def all_pairs():
    """(case id, patient, horizon) of every budget case: 11 patients x 2 horizons"""
    return [(cid, p, h) for cid in CASE_IDS for p in range(len(case(cid)["pts"])) for h in HORIZONS]


_TRUTH, _PROGRAMS = {}, {}


def _key(c, p, prefix, jitter_rounds):
    n = c["pts"][p][1].shape[0]
    return (c["id"], p, _check_prefix(prefix, n).tobytes(), jitter_rounds)


def truth_of(c, p, prefix, jitter_rounds=0):
    """(J, grad) of patient p of a case under a prefix table in long double, computed once per process"""
    key = _key(c, p, prefix, jitter_rounds)
    if key not in _TRUTH:
        m, t, y = c["pts"][p]
        _TRUTH[key] = forecast_grad(*fam(c), m, t, y, c["th"][p], prefix, np.longdouble, jitter_rounds)
    return _TRUTH[key]


def programs_of(c, p, prefix, jitter_rounds=0):
    """dict(truth = (J, grad), en = [E_b, E_c] (objective), eg = [E_b, E_c] (gradient)) of the two fp64 programs"""
    key = _key(c, p, prefix, jitter_rounds)
    if key not in _PROGRAMS:
        m, t, y = c["pts"][p]
        tj, tg = truth_of(c, p, prefix, jitter_rounds)
        b = forecast_grad(*fam(c), m, t, y, c["th"][p], prefix, np.float64, jitter_rounds)
        cc = one_factor(*fam(c), m, t, y, c["th"][p], prefix, jitter_rounds)
        e = [error_pair(b[0], b[1], tj, tg), error_pair(cc[0], cc[1], tj, tg)]
        _PROGRAMS[key] = dict(truth=(tj, tg), en=[x[0] for x in e], eg=[x[1] for x in e])
    return _PROGRAMS[key]


def budget_of(c, p, prefix, jitter_rounds=0):
    """(truth J, truth grad, objective budget, gradient budget) of patient p of a case under a prefix table"""
    r = programs_of(c, p, prefix, jitter_rounds)
    return r["truth"][0], r["truth"][1], min(budget(r["en"], M_OBJ), NLML_BUDGET_CAP), min(budget(r["eg"], M_GRAD), GRAD_BUDGET_CAP)
