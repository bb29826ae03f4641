"""Extended-precision truth of medgp_loo_grad: the negative leave-one-out log pseudo-likelihood and its gradient in the hyper
vector, built on nlml_truth's hyper transforms, Gram matrix, column Cholesky and triangular inverse.  The reference has no such
output: this restatement IS the definition.

    P = K^-1,  alpha = P y,  d_i = P_ii,  u_i = alpha_i / d_i,  s_i = (1 + alpha_i^2 / d_i) / d_i,  v = P u
    log p(y_i | y_-i) = 1/2 log d_i - 1/2 alpha_i^2 / d_i - 1/2 log 2 PI                  (Rasmussen & Williams 5.4.2)
    J = - sum_i log p(y_i | y_-i)
    dJ / d theta_h = 1/2 tr(W_loo dK / d theta_h),     W_loo = P diag(s) P - (alpha v^T + v alpha^T)     (from R&W eq. 5.13)

For LMC-SM the gradient is W_loo through nlml_truth.lmc_grad_naive (one n x n derivative matrix per hyper); for SM and SE the
W -> g lines of nlml_truth.nlml_grad are restated.  form="blocks" takes the block-sum form of nlml_truth.nlml_grad for LMC-SM
instead (test_nlml_truth.py holds the two forms together to 1e-16 in long double): the naive form costs H n^2 long-double
operations, minutes for H = 1114 at n = 512, so patients above NAIVE_MAX_N take the block-sum form.  K is
K + jitter_rounds diag(sigma^2) with the noise gradient NOT scaled, PI = nlml_truth.REF_PI, no prior, any n >= 1 (the call has
no n > 2 guard).

The module also holds the cases shared by tests/test_loo_grad.py (CPU: the budget conditions) and tests/test_loo_grad_gpu.py (the
device held to the budget), the two legitimate fp64 programs the budget is measured on, and the budget constants.
"""
import numpy as np

import nlml_truth as T
from nlml_truth import GRAD_BUDGET_CAP, NLML_BUDGET_CAP, U64, budget, error_pair, spread   # noqa: F401  (the scale nlml uses)

# ---- the budget (measured by tests/test_loo_grad.py::test_budget_factor_M_and_caps on the CPU programs only) ----
# Two legitimate fp64 programs: (b) this code in float64; (c) an fp64 program with another operation order: P = numpy.linalg.inv(K),
# alpha = numpy.linalg.solve(K, y), the gradient in block-sum form.  Starting from nlml's M_NLML = 256 / M_GRAD = 128: the two
# programs stay within M / 4 of each other on every case (worst spread: objective 47.9 -- the SE case --, gradient 5.0 on the cases below,
# errors floored at U64), so the starting values stand.  The budget of a case is M * max(E_b, E_c), floored at M * U64.  Provenance: DESIGN.md section 4.7d.
M_OBJ = 256
M_GRAD = 128
COND_MAX = 1e4             # the inputs are chosen so that the CPU programs alone stay inside the caps: asserted in test_loo_grad.py
NAIVE_MAX_N = 256


def grad_from_w(kidx, Q, D, R, meta, t, theta, W, dtype=np.longdouble, form="naive"):
    """tr(W dK / d theta_h) / 2 for every hyper, W symmetric; the noise component is sigma_d^2 sum_{m_i = d} W_ii whatever the
    jitter (the W -> g lines of nlml_truth.nlml_grad)"""
    X = dtype
    if kidx == 7 and form == "naive":
        return T.lmc_grad_naive(Q, D, R, meta, t, theta, W, X)
    h = T.transform(kidx, Q, D, R, theta, X)
    tt = np.asarray(t, np.float32).astype(X)
    n = tt.shape[0]
    dt = tt[:, None] - tt[None, :]
    g = np.zeros(T.num_hyp(kidx, Q, D, R), X)
    wd = np.diagonal(W)
    if kidx == 7:
        m = np.asarray(meta, np.int64)
        E = np.zeros((n, D), X)
        E[np.arange(n), m] = 1
        g[:D] = h["sig2"] * (wd @ E)
        o_mu, o_v, o_k = D + Q * D * R, D + Q * D * R + Q, D + Q * (D * R + 2)
        for q in range(Q):
            k, km, kv = T._sm_factors(h, q, tt, dt, False)
            S = E.T @ ((W * k) @ E)
            g[D + q * D * R:D + (q + 1) * D * R] = (((S + S.T) / 2) @ h["A"][q]).ravel()
            WB = W * h["B"][q][m[:, None], m[None, :]]
            g[o_mu + q] = np.sum(WB * km) / 2
            g[o_v + q] = np.sum(WB * kv) / 2
            g[o_k + q * D:o_k + (q + 1) * D] = h["kappa"][q] * np.diagonal(S) / 2
    elif kidx == 8:
        g[0] = h["sig2"][0] * np.sum(wd)
        for q in range(Q):
            for j, f in enumerate(T._sm_factors(h, q, tt, dt, False)):
                g[1 + j * Q + q] = h["w"][q] * np.sum(W * f) / 2
    else:
        g[0] = h["sig2"][0] * np.sum(wd)
        r2 = (dt / h["l"]) ** 2
        e = h["sf2"] * np.exp(-r2 / 2)
        g[1] = np.sum(W * e * r2) / 2
        g[2] = np.sum(W * e)
    return g


def _from_inverse(kidx, Q, D, R, meta, t, theta, P, alpha, X, want_grad, form):
    h = T.transform(kidx, Q, D, R, theta, X)
    d = np.diagonal(P).copy()
    q = alpha * alpha / d
    logp = np.log(d) / 2 - q / 2 - np.log(2 * h["pi"]) / 2
    J = -np.sum(logp)
    if not want_grad:
        return J, None, logp
    u = alpha / d
    s = (1 + q) / d
    v = P @ u
    W = (P * s[None, :]) @ P - alpha[:, None] * v[None, :] - v[:, None] * alpha[None, :]
    W = (W + W.T) / 2
    return J, grad_from_w(kidx, Q, D, R, meta, t, theta, W, X, form), logp


def loo_grad(kidx, Q, D, R, meta, t, y, theta, dtype=np.longdouble, jitter_rounds=0, want_grad=True, form=None, want_logp=False):
    """(obj, grad[H] or None) in precision dtype: hand-written column Cholesky, triangular inverse and P = L^-T L^-1 (the same code
    in any dtype).  form: "naive" | "blocks" (LMC-SM only; None = naive up to NAIVE_MAX_N observations)."""
    X = dtype
    t32 = np.asarray(t, np.float32)
    n = t32.shape[0]
    assert n >= 1
    if form is None:
        form = "naive" if n <= NAIVE_MAX_N else "blocks"
    yy = np.asarray(y, np.float32).astype(X)
    K = T.gram(kidx, Q, D, R, meta, t32, theta, X, jitter_rounds)
    Li = T._tri_inverse(T._chol_columns(K))
    P = T._gram_upper_product(Li)
    alpha = Li.T @ (Li @ yy)
    J, g, logp = _from_inverse(kidx, Q, D, R, meta, t32, theta, P, alpha, X, want_grad, form)
    return (J, g, logp) if want_logp else (J, g)


def loo_grad_linalg(kidx, Q, D, R, meta, t, y, theta, jitter_rounds=0):
    """program (c): float64 through numpy.linalg on K (LAPACK's inverse and solve), the gradient in block-sum form"""
    t32 = np.asarray(t, np.float32)
    yy = np.asarray(y, np.float32).astype(np.float64)
    K = T.gram(kidx, Q, D, R, meta, t32, theta, np.float64, jitter_rounds)
    P = np.linalg.inv(K)
    P = (P + P.T) / 2
    alpha = np.linalg.solve(K, yy)
    return _from_inverse(kidx, Q, D, R, meta, t32, theta, P, alpha, np.float64, True, "blocks")[:2]


def cond(kidx, Q, D, R, meta, t, theta, jitter_rounds=0):
    w = np.linalg.eigvalsh(T.gram(kidx, Q, D, R, meta, t, theta, np.float64, jitter_rounds))
    return float(w[-1] / w[0])


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# (id, kidx, Q, D, R, [(n, random_patient mode)]).  Sizes: one observation, the smallest with a gradient of every kind, the 64-block edges
# 63 | 64 | 65, three blocks (130) and four (200, sharing the size class of 130: a ragged class); D = 24 with covariates that have no
# observations; Q = 9 (two launches of the gradient kernel); the single-output families; one patient of the headline shape.
_SPECS = [
    ("lmc_sizes", 7, 2, 3, 2, [(1, "plain"), (3, "plain"), (63, "plain"), (64, "plain"), (65, "shuffled"), (130, "plain"), (200, "plain")]),
    ("lmc_D24_missing", 7, 5, 24, 8, [(130, "missing")]),
    ("lmc_Q9", 7, 9, 3, 2, [(130, "plain")]),
    ("sm_Q4", 8, 4, 1, 0, [(130, None)]),
    ("se", 0, 1, 1, 0, [(130, None)]),
    ("lmc_D24_n512", 7, 5, 24, 8, [(512, "shuffled")]),
]
CASE_IDS = [s[0] for s in _SPECS]
_CASES = {}


def case(cid):
    """dict(id, kidx, Q, D, R, pts = [(meta, t, y)], th = [theta per patient]) from seeds alone"""
    if cid in _CASES:
        return _CASES[cid]
    from medgp_amd import synth
    from random_patients import random_patient
    ci = CASE_IDS.index(cid)
    _, kidx, Q, D, R, spec = _SPECS[ci]
    g = T._philox(20261101, ci)
    pts = []
    for n, mode in spec:
        if kidx == 7:
            pts.append(random_patient(g, D, n, mode))
        else:
            tt = np.sort(g.uniform(0.0, 200.0, size=n)).astype(np.float32)
            pts.append((None, tt, g.standard_normal(n).astype(np.float32)))
    th = [synth.theta(4716, 100 * ci + p, kidx, Q, D, R) for p in range(len(spec))]
    _CASES[cid] = dict(id=cid, kidx=kidx, Q=Q, D=D, R=R, pts=pts, th=th)
    return _CASES[cid]


def fam(c):
    return c["kidx"], c["Q"], c["D"], c["R"]


_TRUTH, _PROGRAMS = {}, {}


def truth_of(c, p, jitter_rounds=0):
    """(obj, grad) of patient p of a case in long double, computed once per process"""
    key = (c["id"], p, jitter_rounds)
    if key not in _TRUTH:
        m, t, y = c["pts"][p]
        _TRUTH[key] = loo_grad(*fam(c), m, t, y, c["th"][p], np.longdouble, jitter_rounds)
    return _TRUTH[key]


def programs_of(c, p, jitter_rounds=0):
    """dict(truth = (obj, grad), en = [E_b, E_c] (objective), eg = [E_b, E_c] (gradient)) of the two fp64 programs"""
    key = (c["id"], p, jitter_rounds)
    if key not in _PROGRAMS:
        m, t, y = c["pts"][p]
        tj, tg = truth_of(c, p, jitter_rounds)
        b = loo_grad(*fam(c), m, t, y, c["th"][p], np.float64, jitter_rounds)
        cc = loo_grad_linalg(*fam(c), m, t, y, c["th"][p], jitter_rounds)
        e = [error_pair(b[0], b[1], tj, tg), error_pair(cc[0], cc[1], tj, tg)]
        _PROGRAMS[key] = dict(truth=(tj, tg), en=[x[0] for x in e], eg=[x[1] for x in e])
    return _PROGRAMS[key]


def budget_of(c, p, jitter_rounds=0):
    """(truth obj, truth grad, objective budget, gradient budget) of patient p of a case"""
    r = programs_of(c, p, jitter_rounds)
    return r["truth"][0], r["truth"][1], min(budget(r["en"], M_OBJ), NLML_BUDGET_CAP), min(budget(r["eg"], M_GRAD), GRAD_BUDGET_CAP)
