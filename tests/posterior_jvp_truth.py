"""Extended-precision truth of medgp_posterior_jvp_batch: the directional derivatives of the posterior mean and variance at test
points along directions in the hyper space, built on nlml_truth's hyper transforms, Gram matrix, column Cholesky and triangular
inverse and on fisher_truth's Kdot.  The reference has no such output: this restatement IS the definition.

    P = (K + jitter_rounds diag(sigma^2))^-1,  alpha = P y,  Kdot = fisher_truth.dgram_dir (the UN-jittered K, noise diagonal included)
    for test point j (covariate m_j, time t*_j):  k_j the column of the cross Gram, kdot_j its derivative along v (no noise term),
    k**_j = sum_q B_q[m_j,m_j],  kdot**_j its derivative,  sigdot_j = 2 sigma^2_{m_j} v_sigma,m_j,  w_j = P k_j,  u = Kdot alpha:
    mean_j = k_j^T alpha                        dmean_j = kdot_j^T alpha - w_j^T u
    var_j  = k**_j - k_j^T P k_j + sigma^2      dvar_j  = kdot**_j + sigdot_j - 2 kdot_j^T w_j + w_j^T Kdot w_j

After k jitter rounds P and alpha belong to K + k diag(sigma^2) while no derivative is scaled by 1 + k: a true derivative at zero
rounds only.  The test times are float32 values, like the training times (the C ABI takes both as float).

The module also holds the cases shared by tests/test_posterior_jvp.py (CPU: the truth and the budget conditions) and
tests/test_posterior_jvp_gpu.py (the device held to the budget) -- the patients of loo_grad_truth._SPECS with fisher_truth's
directions and seeded test points --, the two legitimate fp64 programs the budget is measured on, and the budget constant.
"""
import numpy as np

import fisher_truth as F
import loo_grad_truth as LG
import nlml_truth as T
from fisher_truth import directions   # noqa: F401
from loo_grad_truth import CASE_IDS, COND_MAX, case, cond, fam   # noqa: F401
from nlml_truth import GRAD_BUDGET_CAP, U64, budget, spread   # noqa: F401

# ---- the budget (measured by tests/test_posterior_jvp.py::test_budget_factor_M_and_caps on the CPU programs only) ----
# Two legitimate fp64 programs: (b) this code in float64; (c) P = numpy.linalg.inv(K), alpha = numpy.linalg.solve(K, y).  Starting from
# the project's M_GRAD = 128: the two programs stay within M / 4 of each other on every case, so the starting value stands.  The
# budget of a case is M_PJVP * max(E_b, E_c), floored at M_PJVP * U64, capped at GRAD_BUDGET_CAP.  The error scale is the magnitude
# of the terms of each output (mags), not the output: both are differences of terms that cancel.  Provenance: DESIGN.md section 4.7o.
M_PJVP = 128
NVEC = 2
POINT_COUNTS = [0, 1, 63, 64, 65, 130]     # test points per patient: every edge of the 64-point tile is met ...
# ... by the patients of the cases in this order (lmc_sizes: n = 1, 3, 63, 64, 65, 130, 200)
CASE_POINTS = {"lmc_sizes": [1, 0, 63, 64, 65, 130, 64], "lmc_D24_missing": [130], "lmc_Q9": [65], "sm_Q4": [130], "se": [65], "lmc_D24_n512": [64]}
OUTSIDE_H = 24.0                           # test times reach this far outside the observed range


def _meta(kidx, meta, n):
    return np.asarray(meta, np.int64) if kidx == 7 else np.zeros(n, np.int64)


def cross_gram(kidx, Q, D, R, meta, t, theta, meta2, t2, dtype=np.longdouble):
    """(K* [n, m], k** [m] without noise, sigma^2 of the test points' covariates [m]) in precision dtype"""
    X = dtype
    h = T.transform(kidx, Q, D, R, theta, X)
    tt = np.asarray(t, np.float32).astype(X)
    t2 = np.asarray(t2, np.float32).astype(X)
    n, mm = tt.shape[0], t2.shape[0]
    m, m2 = _meta(kidx, meta, n), _meta(kidx, meta2, mm)
    dt = tt[:, None] - t2[None, :]
    Ks, kss = np.zeros((n, mm), X), np.zeros(mm, X)
    if kidx == 0:
        Ks += h["sf2"] * np.exp(-(dt / h["l"]) ** 2 / 2)
        kss += h["sf2"]
    else:
        for q in range(Q):
            k = T._sm_factors(h, q, tt, dt, False)[0]
            if kidx == 7:
                Ks += h["B"][q][m[:, None], m2[None, :]] * k
                kss += h["B"][q][m2, m2]
            else:
                Ks += h["w"][q] * k
                kss += h["w"][q]
    return Ks, kss, h["sig2"][m2]


def dcross_gram_dir(kidx, Q, D, R, meta, t, theta, meta2, t2, v, dtype=np.longdouble):
    """(Kdot* [n, m], kdot** [m], sigdot [m]): the derivatives of cross_gram's three outputs along v (fisher_truth.dgram_dir's formulas
    on the cross pairs; no noise term in the first two)"""
    X = dtype
    h = T.transform(kidx, Q, D, R, theta, X)
    vv = np.asarray(v).astype(X)
    assert vv.shape == (T.num_hyp(kidx, Q, D, R),), vv.shape
    tt = np.asarray(t, np.float32).astype(X)
    t2 = np.asarray(t2, np.float32).astype(X)
    n, mm = tt.shape[0], t2.shape[0]
    m, m2 = _meta(kidx, meta, n), _meta(kidx, meta2, mm)
    dt = tt[:, None] - t2[None, :]
    Kd, kd = np.zeros((n, mm), X), np.zeros(mm, X)
    if kidx == 7:
        c = vv[D:]
        Ad = c[:Q * D * R].reshape(Q, D, R)
        vmu, vv_, vk = c[Q * D * R:Q * D * R + Q], c[Q * D * R + Q:Q * D * R + 2 * Q], c[Q * (D * R + 2):].reshape(Q, D)
        for q in range(Q):
            k, km, kv = T._sm_factors(h, q, tt, dt, False)
            Bd = Ad[q] @ h["A"][q].T + h["A"][q] @ Ad[q].T
            Bd[np.arange(D), np.arange(D)] += h["kappa"][q] * vk[q]
            Kd += Bd[m[:, None], m2[None, :]] * k + h["B"][q][m[:, None], m2[None, :]] * (vmu[q] * km + vv_[q] * kv)
            kd += Bd[m2, m2]
    elif kidx == 8:
        for q in range(Q):
            k, km, kv = T._sm_factors(h, q, tt, dt, False)
            Kd += h["w"][q] * (vv[1 + q] * k + vv[1 + Q + q] * km + vv[1 + 2 * Q + q] * kv)
            kd += h["w"][q] * vv[1 + q]
    else:
        r2 = (dt / h["l"]) ** 2
        e = h["sf2"] * np.exp(-r2 / 2)
        Kd += vv[1] * e * r2 + 2 * vv[2] * e
        kd += 2 * vv[2] * h["sf2"]
    nl = D if kidx == 7 else 1
    return Kd, kd, 2 * h["sig2"][m2] * vv[:nl][m2]


def parts(kidx, Q, D, R, meta, t, y, theta, dtype=np.longdouble, jitter_rounds=0):
    """(P, alpha) in precision dtype: column Cholesky, triangular inverse, L^-T L^-1"""
    X = dtype
    K = T.gram(kidx, Q, D, R, meta, np.asarray(t, np.float32), theta, X, jitter_rounds)
    Li = T._tri_inverse(T._chol_columns(K))
    return T._gram_upper_product(Li), Li.T @ (Li @ np.asarray(y, np.float32).astype(X))


def parts_linalg(kidx, Q, D, R, meta, t, y, theta, jitter_rounds=0):
    """program (c): float64 through numpy.linalg on K (LAPACK's inverse and solve)"""
    K = T.gram(kidx, Q, D, R, meta, np.asarray(t, np.float32), theta, np.float64, jitter_rounds)
    P = np.linalg.inv(K)
    return (P + P.T) / 2, np.linalg.solve(K, np.asarray(y, np.float32).astype(np.float64))


def posterior_from_parts(kidx, Q, D, R, meta, t, theta, meta2, t2, P, alpha, dtype=np.longdouble):
    """(mean [m], var [m]): the plug-in posterior, the noise of the test points' covariates added once, no clamp"""
    Ks, kss, s2 = cross_gram(kidx, Q, D, R, meta, t, theta, meta2, t2, dtype)
    return Ks.T @ alpha, kss - np.sum(Ks * (P @ Ks), axis=0) + s2


def posterior(kidx, Q, D, R, meta, t, y, theta, meta2, t2, dtype=np.longdouble, jitter_rounds=0):
    P, alpha = parts(kidx, Q, D, R, meta, t, y, theta, dtype, jitter_rounds)
    return posterior_from_parts(kidx, Q, D, R, meta, t, theta, meta2, t2, P, alpha, dtype)


def jvp_from_parts(kidx, Q, D, R, meta, t, theta, meta2, t2, P, alpha, vecs, dtype=np.longdouble, want_mag=False):
    """(dmean [m, nvec], dvar [m, nvec]) from given P and alpha; want_mag: also mags' two arrays of the same shape"""
    X = dtype
    t32 = np.asarray(t, np.float32)
    Ks = cross_gram(kidx, Q, D, R, meta, t32, theta, meta2, t2, X)[0]
    Wm = P @ Ks                                    # column j is w_j
    V = np.atleast_2d(np.asarray(vecs))
    mm = Ks.shape[1]
    dmean, dvar = np.zeros((mm, V.shape[0]), X), np.zeros((mm, V.shape[0]), X)
    gm, gv = np.zeros_like(dmean), np.zeros_like(dvar)
    for k, v in enumerate(V):
        Kd = F.dgram_dir(kidx, Q, D, R, meta, t32, theta, v, X)
        Kds, kd, sd = dcross_gram_dir(kidx, Q, D, R, meta, t32, theta, meta2, t2, v, X)
        u = Kd @ alpha
        Y = Kd @ Wm
        dmean[:, k] = Kds.T @ alpha - Wm.T @ u
        dvar[:, k] = kd + sd - 2 * np.sum(Kds * Wm, axis=0) + np.sum(Wm * Y, axis=0)
        gm[:, k] = np.abs(Kds).T @ np.abs(alpha) + np.abs(Wm).T @ np.abs(u)
        gv[:, k] = np.abs(kd) + np.abs(sd) + 2 * np.sum(np.abs(Kds * Wm), axis=0) + np.sum(np.abs(Wm * Y), axis=0)
    return (dmean, dvar, gm, gv) if want_mag else (dmean, dvar)


def jvp(kidx, Q, D, R, meta, t, y, theta, meta2, t2, vecs, dtype=np.longdouble, jitter_rounds=0):
    """(dmean [m, nvec], dvar [m, nvec]) for the rows of vecs ([nvec, H] or [H]) in precision dtype"""
    P, alpha = parts(kidx, Q, D, R, meta, t, y, theta, dtype, jitter_rounds)
    return jvp_from_parts(kidx, Q, D, R, meta, t, theta, meta2, t2, P, alpha, vecs, dtype)


def mags(kidx, Q, D, R, meta, t, y, theta, meta2, t2, vecs, dtype=np.longdouble, jitter_rounds=0):
    """(mag_mean [m, nvec], mag_var [m, nvec]): per point the sums of the absolute values of the terms,
    mag_mean_j = sum_i |kdot_ij alpha_i| + sum_i |w_ij u_i|,   mag_var_j = |kdot**| + |sigdot| + 2 sum_i |kdot_ij w_ij| + sum_i |w_ij (Kdot w)_ij|"""
    P, alpha = parts(kidx, Q, D, R, meta, t, y, theta, dtype, jitter_rounds)
    return jvp_from_parts(kidx, Q, D, R, meta, t, theta, meta2, t2, P, alpha, vecs, dtype, True)[2:]


def jvp_linalg(kidx, Q, D, R, meta, t, y, theta, meta2, t2, vecs, jitter_rounds=0):
    P, alpha = parts_linalg(kidx, Q, D, R, meta, t, y, theta, jitter_rounds)
    return jvp_from_parts(kidx, Q, D, R, meta, t, theta, meta2, t2, P, alpha, vecs, np.float64)


# ---- errors ------------------------------------------------------------------------------------------------------------------------

def scale_of(mag):
    """the error scale of one output array: the magnitude of each point's terms, floored at 1e-3 of the largest"""
    mg = np.asarray(mag, np.longdouble)
    return np.maximum(mg, np.longdouble(1e-3) * mg.max()) if mg.size else mg


def error_of(got, truth, mag):
    """E = max_j |x_j - truth_j| / max(mag_j, 1e-3 max_j mag_j), per direction, worst over the directions; NaN gives inf"""
    got, truth, mag = np.asarray(got), np.asarray(truth), np.asarray(mag)
    assert got.shape == truth.shape == mag.shape, (got.shape, truth.shape, mag.shape)
    worst = 0.0
    if got.size == 0:
        return worst
    for k in range(got.shape[1]):
        e = np.abs(got[:, k].astype(np.float64).astype(np.longdouble) - truth[:, k]) / scale_of(mag[:, k])
        worst = max(worst, float("inf") if np.isnan(e).any() else float(e.max()))
    return worst


def errors(got, truth):
    """the larger of the dmean and the dvar error; got = (dmean, dvar), truth = (dmean, dvar, mag_mean, mag_var)"""
    return max(error_of(got[0], truth[0], truth[2]), error_of(got[1], truth[1], truth[3]))


# ---- the cases -------------------------------------------------------------------------------------------------------------------

def patients():
    """[(case id, patient index)] of every patient of every case, in order"""
    return [(cid, p) for cid in CASE_IDS for p in range(len(case(cid)["pts"]))]


def points(c, p, count=None):
    """(meta2 or None, t2 float32) of patient p of a case, from seeds alone: CASE_POINTS of them (count: another number, for the tests
    that need one), times uniform from OUTSIDE_H before the first to OUTSIDE_H after the last observation; LMC-SM: covariates uniform
    over all D -- for `missing` patients that includes covariates without an observation."""
    ci = CASE_IDS.index(c["id"])
    if count is None:
        count = CASE_POINTS[c["id"]][p]
    g = T._philox(20261501, 1000 * ci + p)
    t = np.asarray(c["pts"][p][1], np.float32)
    t2 = g.uniform(float(t.min()) - OUTSIDE_H, float(t.max()) + OUTSIDE_H, size=count).astype(np.float32)
    m2 = g.integers(0, c["D"], size=count).astype(np.int32) if c["kidx"] == 7 else None
    return m2, t2


_TRUTH, _PROGRAMS = {}, {}


def truth_of(c, p, jitter_rounds=0, nvec=NVEC, count=None):
    """(dmean, dvar, mag_mean, mag_var), each [m, nvec], in long double, computed once per process"""
    key = (c["id"], p, jitter_rounds, nvec, count)
    if key not in _TRUTH:
        m, t, y = c["pts"][p]
        m2, t2 = points(c, p, count)
        P, alpha = parts(*fam(c), m, t, y, c["th"][p], np.longdouble, jitter_rounds)
        _TRUTH[key] = jvp_from_parts(*fam(c), m, t, c["th"][p], m2, t2, P, alpha, directions(c, p, nvec), np.longdouble, True)
    return _TRUTH[key]


def programs_of(c, p, jitter_rounds=0, count=None):
    """dict(truth = (dmean, dvar, mag_mean, mag_var), eg = [E_b, E_c]) of the two fp64 programs.  A patient without points has no
    error to measure: its programs count as exact (the floor U64 then sets the budget, and nothing is compared against it)."""
    key = (c["id"], p, jitter_rounds, count)
    if key not in _PROGRAMS:
        m, t, y = c["pts"][p]
        m2, t2 = points(c, p, count)
        tr = truth_of(c, p, jitter_rounds, count=count)
        V = directions(c, p)
        b = jvp(*fam(c), m, t, y, c["th"][p], m2, t2, V, np.float64, jitter_rounds)
        cc = jvp_linalg(*fam(c), m, t, y, c["th"][p], m2, t2, V, jitter_rounds)
        _PROGRAMS[key] = dict(truth=tr, eg=[errors(b, tr), errors(cc, tr)])
    return _PROGRAMS[key]


def budget_of(c, p, jitter_rounds=0, count=None):
    """(truth tuple, budget) of patient p of a case"""
    r = programs_of(c, p, jitter_rounds, count)
    return r["truth"], min(budget(r["eg"], M_PJVP), GRAD_BUDGET_CAP)
