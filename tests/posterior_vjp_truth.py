"""Extended-precision truth of medgp_posterior_vjp_batch: the gradient in the hypers of a loss of the posterior mean and variance at
test points, for given cotangents cm_j = dloss / dmean_j, cv_j = dloss / dvar_j.  The reference has no such output.

THE DEFINITION is the identity with the JVP: grad_h = sum_j cm_j dmean_j(e_h) + cv_j dvar_j(e_h), with dmean, dvar those of
posterior_jvp_truth.jvp on the unit direction e_h (by_definition below, long double).  It costs H directions, so the cases are held
against the independent CLOSED FORM (closed_form below: same code in any dtype), which tests/test_posterior_vjp.py holds to the
definition -- on every hyper of the small cases and on a seeded subset of hypers of the D = 24 cases:

    W = P K*,  c = W cm,  Wc = W diag(cv),
    grad_h = 1/2 tr(G dK/dtheta_h) + sum_ij R_ij dk*_ij/dtheta_h + sum_j cv_j (dk**_j/dtheta_h + 2 sigma^2_{m_j} [h = sigma_{m_j}])
    G = 2 Wc W^T - (c alpha^T + alpha c^T),   R = alpha cm^T - 2 Wc,

dK the derivative of the UN-jittered kernel with its noise diagonal (after k jitter rounds P and alpha belong to K + k diag(sigma^2)
and no derivative is scaled by 1 + k, as in the JVP).  The error scale of line h is the sum of the absolute values of its terms
(the same code run on |G|, |R|, |cv| and the absolute values of every kernel factor and coefficient), floored at 1e-3 of the largest,
as posterior_jvp_truth.mags does for the forward mode.

The module also holds the cases shared by tests/test_posterior_vjp.py and tests/test_posterior_vjp_gpu.py -- the patients of
loo_grad_truth._SPECS with posterior_jvp_truth's test points (lmc_D24_missing: edited so that one observed covariate has no test
point and one unobserved covariate has some) and seeded cotangents --, the two legitimate fp64 programs and the budget constant.
"""
import numpy as np

import loo_grad_truth as LG
import nlml_truth as T
import posterior_jvp_truth as PJ
from loo_grad_truth import CASE_IDS, case, fam   # noqa: F401
from nlml_truth import GRAD_BUDGET_CAP, U64, budget, spread   # noqa: F401
from posterior_jvp_truth import CASE_POINTS   # noqa: F401

# ---- the budget (measured by tests/test_posterior_vjp.py::test_budget_factor_M_and_caps on the CPU programs only) ----
# Two legitimate fp64 programs: (b) closed_form in float64 on this file's Cholesky route; (c) the same on P = numpy.linalg.inv(K),
# alpha = numpy.linalg.solve(K, y).  Starting from the project's M_GRAD = 128.  Measured over all cases, one jitter round included
# (errors floored at U64): the largest spread of the two programs is 3.6 (lmc_sizes, n = 130, one jitter round) <= M / 4 = 32, so the starting
# value stands.  The device is no part of it.  Provenance: DESIGN.md section 4.7p.
M_PVJP = 128
NCOT = 2
MEASURED_SPREAD = 3.6


def _meta(kidx, meta, n):
    return np.asarray(meta, np.int64) if kidx == 7 else np.zeros(n, np.int64)


def _lines(kidx, Q, D, R, meta, t, theta, meta2, t2, G, Rm, cv, X, absolute=False):
    """The H lines  1/2 sum_ij G_ij dK_ij/dtheta_h + sum_ij Rm_ij dk*_ij/dtheta_h + sum_j cv_j (dk**_j + dsigma^2_{m_j})/dtheta_h  in
    precision X.  absolute: every factor by its absolute value -- the sum of the absolute values of the terms (an upper bound of it
    where a coefficient is itself a sum: B_q = A_q A_q^T + kappa_q is taken as |A_q| |A_q|^T + kappa_q)."""
    ab = np.abs if absolute else (lambda x: x)
    h = T.transform(kidx, Q, D, R, theta, X)
    tt = np.asarray(t, np.float32).astype(X)
    ts = np.asarray(t2, np.float32).astype(X)
    n, mm = tt.shape[0], ts.shape[0]
    m, m2 = _meta(kidx, meta, n), _meta(kidx, meta2, mm)
    G, Rm, cv = ab(np.asarray(G, X)), ab(np.asarray(Rm, X)), ab(np.asarray(cv, X))
    dt, ds = tt[:, None] - tt[None, :], tt[:, None] - ts[None, :]
    nl = D if kidx == 7 else 1
    E, E2 = np.zeros((n, nl), X), np.zeros((mm, nl), X)
    E[np.arange(n), m] = 1
    E2[np.arange(mm), m2] = 1
    cvs = cv @ E2                                   # per covariate: sum of cv over its test points
    g = np.zeros(T.num_hyp(kidx, Q, D, R), X)
    g[:nl] = h["sig2"] * (np.diagonal(G) @ E) + 2 * h["sig2"] * cvs
    if kidx == 7:
        o_mu, o_v, o_k = D + Q * D * R, D + Q * D * R + Q, D + Q * (D * R + 2)
        for q in range(Q):
            A = ab(h["A"][q])
            B = A @ A.T + np.diag(h["kappa"][q]) if absolute else h["B"][q]
            k, km, kv = [ab(f) for f in T._sm_factors(h, q, tt, dt, False)]
            ks, kms, kvs = [ab(f) for f in T._sm_factors(h, q, tt, ds, False)]
            S = E.T @ ((G * k) @ E)                 # [D, D], symmetric up to rounding
            Xc = E.T @ ((Rm * ks) @ E2)             # [D, D], not symmetric
            full = (S + S.T) / 2 + (Xc + Xc.T) + 2 * np.diag(cvs)   # dB_q is symmetric: the coefficient of dB_q[d,e] / 2 ... times 2
            g[D + q * D * R:D + (q + 1) * D * R] = (full @ A).ravel()
            g[o_k + q * D:o_k + (q + 1) * D] = h["kappa"][q] * np.diagonal(full) / 2
            Bg, Bs = B[m[:, None], m[None, :]], B[m[:, None], m2[None, :]]
            g[o_mu + q] = np.sum(G * Bg * km) / 2 + np.sum(Rm * Bs * kms)
            g[o_v + q] = np.sum(G * Bg * kv) / 2 + np.sum(Rm * Bs * kvs)
    elif kidx == 8:
        for q in range(Q):
            f, fs = T._sm_factors(h, q, tt, dt, False), T._sm_factors(h, q, tt, ds, False)
            for j in range(3):
                g[1 + j * Q + q] = h["w"][q] * (np.sum(G * ab(f[j])) / 2 + np.sum(Rm * ab(fs[j])))
            g[1 + q] += h["w"][q] * cvs[0]
    else:
        r2, r2s = (dt / h["l"]) ** 2, (ds / h["l"]) ** 2
        e, es = h["sf2"] * np.exp(-r2 / 2), h["sf2"] * np.exp(-r2s / 2)
        g[1] = np.sum(G * e * r2) / 2 + np.sum(Rm * es * r2s)
        g[2] = np.sum(G * e) + 2 * np.sum(Rm * es) + 2 * h["sf2"] * cvs[0]
    return g


def _sets(a, mm, X):
    """cotangents [m] or [m, ncot] -> [m, ncot] in precision X (m = 0 keeps the number of sets of a 2-d input)"""
    a = np.asarray(a, np.float64).astype(X)
    return a.reshape(mm, a.shape[1] if a.ndim == 2 else 1)


def closed_from_parts(kidx, Q, D, R, meta, t, theta, meta2, t2, P, alpha, cm, cv, dtype=np.longdouble, want_mag=False):
    """grad [ncot, H] (and mag [ncot, H]) from given P and alpha; cm, cv: [m] or [m, ncot]"""
    X = dtype
    Ks = PJ.cross_gram(kidx, Q, D, R, meta, np.asarray(t, np.float32), theta, meta2, t2, X)[0]
    W = P @ Ks
    cm, cv = _sets(cm, Ks.shape[1], X), _sets(cv, Ks.shape[1], X)
    out, mag = [], []
    for k in range(cm.shape[1]):
        c, Wc = W @ cm[:, k], W * cv[None, :, k]
        t1, t2_, t3 = 2 * (Wc @ W.T), np.outer(c, alpha), np.outer(alpha, c)
        G = t1 - (t2_ + t3)
        G = (G + G.T) / 2
        r1, r2 = np.outer(alpha, cm[:, k]), 2 * Wc
        out.append(_lines(kidx, Q, D, R, meta, t, theta, meta2, t2, G, r1 - r2, cv[:, k], X))
        if want_mag:
            Ga = np.abs(np.abs(Wc) @ np.abs(W.T)) * 2 + np.abs(t2_) + np.abs(t3)
            mag.append(_lines(kidx, Q, D, R, meta, t, theta, meta2, t2, Ga, np.abs(r1) + np.abs(r2), cv[:, k], X, True))
    return (np.array(out), np.array(mag)) if want_mag else np.array(out)


def closed_form(kidx, Q, D, R, meta, t, y, theta, meta2, t2, cm, cv, dtype=np.longdouble, jitter_rounds=0):
    P, alpha = PJ.parts(kidx, Q, D, R, meta, t, y, theta, dtype, jitter_rounds)
    return closed_from_parts(kidx, Q, D, R, meta, t, theta, meta2, t2, P, alpha, cm, cv, dtype)


def closed_form_linalg(kidx, Q, D, R, meta, t, y, theta, meta2, t2, cm, cv, jitter_rounds=0):
    P, alpha = PJ.parts_linalg(kidx, Q, D, R, meta, t, y, theta, jitter_rounds)
    return closed_from_parts(kidx, Q, D, R, meta, t, theta, meta2, t2, P, alpha, cm, cv, np.float64)


def by_definition(kidx, Q, D, R, meta, t, y, theta, meta2, t2, cm, cv, hypers=None, dtype=np.longdouble, jitter_rounds=0):
    """grad [ncot, |hypers|] by the JVP on unit directions (hypers: indices, default all H)"""
    X = dtype
    H = T.num_hyp(kidx, Q, D, R)
    hs = np.arange(H) if hypers is None else np.asarray(hypers, np.int64)
    V = np.zeros((hs.shape[0], H))
    V[np.arange(hs.shape[0]), hs] = 1.0
    dmean, dvar = PJ.jvp(kidx, Q, D, R, meta, t, y, theta, meta2, t2, V, X, jitter_rounds)   # [m, |hs|]
    cm, cv = _sets(cm, dmean.shape[0], X), _sets(cv, dmean.shape[0], X)
    return cm.T @ dmean + cv.T @ dvar


# ---- errors ------------------------------------------------------------------------------------------------------------------------

def error_of(got, truth, mag):
    """E = max_h |g_h - truth_h| / max(mag_h, 1e-3 max mag), per cotangent set, worst over the sets; NaN gives inf"""
    got, truth, mag = np.atleast_2d(np.asarray(got)), np.atleast_2d(np.asarray(truth)), np.atleast_2d(np.asarray(mag))
    assert got.shape == truth.shape == mag.shape, (got.shape, truth.shape, mag.shape)
    worst = 0.0
    for k in range(got.shape[0]):
        if not mag[k].max() > 0:      # no points: the gradient is exactly zero
            e = np.abs(got[k].astype(np.float64).astype(np.longdouble) - truth[k])
            worst = max(worst, float("inf") if (np.isnan(e).any() or e.max() > 0) else 0.0)
            continue
        e = np.abs(got[k].astype(np.float64).astype(np.longdouble) - truth[k]) / PJ.scale_of(mag[k])
        worst = max(worst, float("inf") if np.isnan(e).any() else float(e.max()))
    return worst


# ---- the cases -------------------------------------------------------------------------------------------------------------------

def patients():
    return PJ.patients()


def points(c, p, count=None):
    """(meta2 or None, t2) of patient p: posterior_jvp_truth.points; for lmc_D24_missing (default count) edited so that (a) the
    smallest observed covariate has NO test point and (b) the smallest unobserved covariate has two."""
    m2, t2 = PJ.points(c, p, count)
    if c["id"] == "lmc_D24_missing" and count is None:
        obs = set(int(x) for x in np.asarray(c["pts"][p][0]))
        a = min(obs)
        b = min(d for d in range(c["D"]) if d not in obs)
        keep = m2 != a
        m2, t2 = m2[keep], t2[keep]
        m2 = np.concatenate([m2[:5], [b], m2[5:], [b]]).astype(np.int32)
        t2 = np.concatenate([t2[:5], [t2[0] + np.float32(0.5)], t2[5:], [t2[1] + np.float32(0.25)]]).astype(np.float32)
    return m2, t2


def cotangents(c, p, ncot=NCOT, count=None):
    """(cm [m, ncot], cv [m, ncot]) from seeds alone: standard normal"""
    ci = CASE_IDS.index(c["id"])
    mm = points(c, p, count)[1].shape[0]
    g = T._philox(20261601, 1000 * ci + p)
    z = g.standard_normal((2, max(mm, 1), 8))[:, :mm, :ncot]
    return np.ascontiguousarray(z[0]), np.ascontiguousarray(z[1])


def targets(c, p, count=None):
    """(y2 [m], wt [m]) for the built-in losses: seeded, y2 within a few units of the data's scale, wt in [0.5, 1.5]"""
    ci = CASE_IDS.index(c["id"])
    mm = points(c, p, count)[1].shape[0]
    g = T._philox(20261602, 1000 * ci + p)
    return g.standard_normal(mm), g.uniform(0.5, 1.5, size=mm)


_TRUTH, _PROGRAMS, _POST = {}, {}, {}


def posterior_of(c, p, jitter_rounds=0, count=None):
    """(mean, var) in long double"""
    key = (c["id"], p, jitter_rounds, count)
    if key not in _POST:
        m, t, y = c["pts"][p]
        m2, t2 = points(c, p, count)
        _POST[key] = PJ.posterior(*fam(c), m, t, y, c["th"][p], m2, t2, np.longdouble, jitter_rounds)
    return _POST[key]


def truth_for(c, p, cm, cv, jitter_rounds=0, count=None):
    """(grad [ncot, H], mag [ncot, H]) in long double for given cotangents (not cached)"""
    m, t, y = c["pts"][p]
    m2, t2 = points(c, p, count)
    P, alpha = PJ.parts(*fam(c), m, t, y, c["th"][p], np.longdouble, jitter_rounds)
    return closed_from_parts(*fam(c), m, t, c["th"][p], m2, t2, P, alpha, cm, cv, np.longdouble, True)


def truth_of(c, p, jitter_rounds=0, ncot=NCOT, count=None):
    """(grad [ncot, H], mag [ncot, H]) for the seeded cotangents, computed once per process"""
    key = (c["id"], p, jitter_rounds, ncot, count)
    if key not in _TRUTH:
        cm, cv = cotangents(c, p, ncot, count)
        _TRUTH[key] = truth_for(c, p, cm, cv, jitter_rounds, count)
    return _TRUTH[key]


def programs_of(c, p, jitter_rounds=0, count=None):
    """dict(truth = (grad, mag), eg = [E_b, E_c]) of the two fp64 programs on the seeded cotangents"""
    key = (c["id"], p, jitter_rounds, count)
    if key not in _PROGRAMS:
        m, t, y = c["pts"][p]
        m2, t2 = points(c, p, count)
        cm, cv = cotangents(c, p, NCOT, count)
        tr = truth_of(c, p, jitter_rounds, count=count)
        b = closed_form(*fam(c), m, t, y, c["th"][p], m2, t2, cm, cv, np.float64, jitter_rounds)
        cc = closed_form_linalg(*fam(c), m, t, y, c["th"][p], m2, t2, cm, cv, jitter_rounds)
        _PROGRAMS[key] = dict(truth=tr, eg=[error_of(b, tr[0], tr[1]), error_of(cc, tr[0], tr[1])])
    return _PROGRAMS[key]


def budget_of(c, p, jitter_rounds=0, count=None):
    """(truth (grad, mag), budget) of patient p of a case: the budget of its seeded cotangents, which every other cotangent set of
    the same patient is held to as well (the error scale follows the set)"""
    r = programs_of(c, p, jitter_rounds, count)
    return r["truth"], min(budget(r["eg"], M_PVJP), GRAD_BUDGET_CAP)


def groups_nonzero(c, mag_or_grad):
    """True when the array has a non-zero entry in each of the noise, coefficient (A / w / sf), mu and v groups of the family"""
    from medgp_amd.sensitivity import groups
    x = np.atleast_2d(np.asarray(mag_or_grad))
    want = {7: ["noise", "A", "mu", "v"], 8: ["noise", "w", "mu", "v"], 0: ["noise", "l", "sf"]}[c["kidx"]]
    gs = dict(groups(*fam(c)))
    return all(bool(np.any(x[:, gs[n]] != 0)) for n in want)
