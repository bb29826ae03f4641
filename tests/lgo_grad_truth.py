"""Extended-precision truth of medgp_lgo_grad: the negative leave-group-out log pseudo-likelihood and its gradient in the hyper
vector, built on nlml_truth's hyper transforms, Gram matrix, column Cholesky and triangular inverse and on
loo_grad_truth.grad_from_w.  The reference has no such output: this restatement IS the definition.

    K the matrix that is factored (noise included, jitter_rounds diag(sigma^2) added),  P = K^-1,  alpha = P y
    for every non-empty group g >= 0 with the ascending index set B:
        M_g = P[B, B],   r_g = M_g^-1 alpha_B,   lpd_g = -1/2 alpha_B^T r_g + 1/2 log det M_g - |B| / 2 log 2 PI
    J = - sum_g lpd_g
    S = sum_g E_g (M_g^-1 + r_g r_g^T) E_g^T,   r = sum_g E_g r_g,   v = P r
    dJ / d theta_h = 1/2 tr(W_lgo dK / d theta_h),     W_lgo = P S P - (alpha v^T + v alpha^T)

(d lpd_g = 1/2 tr(M^-1 dM) - alpha_B^T M^-1 d alpha_B + 1/2 r^T dM r with dP = -P dK P and d alpha = -P dK alpha.)  Observations
with id -1 are never held out.  PI = nlml_truth.REF_PI, no prior, any n >= 1.  The gradient takes the per-hyper trace up to
NAIVE_MAX_N observations and the block-sum form above (loo_grad_truth.grad_from_w).

The module also holds the cases shared by tests/test_lgo_grad.py (CPU: the budget conditions) and tests/test_lgo_grad_gpu.py (the
device held to the budget), the two legitimate fp64 programs the budget is measured on, and the budget constants.
"""
import numpy as np

import loo_grad_truth as LG
import nlml_truth as T
from loo_grad_truth import COND_MAX, NAIVE_MAX_N, cond, fam, grad_from_w   # noqa: F401
from nlml_truth import GRAD_BUDGET_CAP, NLML_BUDGET_CAP, U64, budget, error_pair, spread   # noqa: F401

# ---- the budget (measured by tests/test_lgo_grad.py::test_budget_factor_M_and_caps on the CPU programs only) ----
# Two legitimate fp64 programs: (b) this code in float64; (c) numpy.linalg.inv / solve on K and on every M_g, the gradient in block-sum
# form.  Starting from the project's M_OBJ = 256 / M_GRAD = 128: the two programs stay within M / 4 of each other on every case below
# (worst spread measured: objective 18.3, gradient 8.8, errors floored at U64), so the starting values stand.  The budget of a
# case is M * max(E_b, E_c), floored at M * U64.  Provenance: DESIGN.md section 4.7l.
M_OBJ = 256
M_GRAD = 128


def _group_inverse(M, X):
    """(M^-1, log det M) in precision X by the hand-written column Cholesky"""
    L = T._chol_columns(M)
    Li = T._tri_inverse(L)
    return T._gram_upper_product(Li), 2 * np.sum(np.log(np.diagonal(L)))


def _group_inverse_linalg(M, X):
    Mi = np.linalg.inv(M)
    return (Mi + Mi.T) / 2, np.linalg.slogdet(M)[1]


def _from_inverse(kidx, Q, D, R, meta, t, theta, P, alpha, group, ngroups, X, want_grad, form, inverse):
    h = T.transform(kidx, Q, D, R, theta, X)
    n = P.shape[0]
    ids = np.asarray(group, np.int64)
    assert ids.shape == (n,) and ids.min() >= -1 and ids.max() < ngroups
    lpd = np.zeros(ngroups, X)
    S = np.zeros((n, n), X)
    r = np.zeros(n, X)
    for g in range(ngroups):
        B = np.flatnonzero(ids == g)
        if B.size == 0:
            continue
        Mi, logdet = inverse(P[np.ix_(B, B)].copy(), X)
        rg = Mi @ alpha[B]
        lpd[g] = -(alpha[B] @ rg) / 2 + logdet / 2 - B.size * np.log(2 * h["pi"]) / 2
        if want_grad:
            S[np.ix_(B, B)] = Mi + rg[:, None] * rg[None, :]
            r[B] = rg
    J = -np.sum(lpd)
    if not want_grad:
        return J, None, lpd
    v = P @ r
    W = P @ (S @ P) - alpha[:, None] * v[None, :] - v[:, None] * alpha[None, :]
    W = (W + W.T) / 2
    return J, grad_from_w(kidx, Q, D, R, meta, t, theta, W, X, form), lpd


def lgo_grad(kidx, Q, D, R, meta, t, y, theta, group, ngroups, dtype=np.longdouble, jitter_rounds=0, want_grad=True, form=None, want_lpd=False):
    """(obj, grad[H] or None) in precision dtype: hand-written column Cholesky, triangular inverse and P = L^-T L^-1 of K and of every
    M_g (the same code in any dtype).  form: "naive" | "blocks" (LMC-SM only; None = naive up to NAIVE_MAX_N observations)."""
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
    J, g, lpd = _from_inverse(kidx, Q, D, R, meta, t32, theta, P, alpha, group, ngroups, X, want_grad, form, _group_inverse)
    return (J, g, lpd) if want_lpd else (J, g)


def lgo_grad_linalg(kidx, Q, D, R, meta, t, y, theta, group, ngroups, jitter_rounds=0):
    """program (c): float64 through numpy.linalg on K and on every M_g (LAPACK's inverse and solve), the gradient in block-sum form"""
    t32 = np.asarray(t, np.float32)
    yy = np.asarray(y, np.float32).astype(np.float64)
    K = T.gram(kidx, Q, D, R, meta, t32, theta, np.float64, jitter_rounds)
    P = np.linalg.inv(K)
    P = (P + P.T) / 2
    alpha = np.linalg.solve(K, yy)
    return _from_inverse(kidx, Q, D, R, meta, t32, theta, P, alpha, group, ngroups, np.float64, True, "blocks", _group_inverse_linalg)[:2]


# ---- the group schemes -----------------------------------------------------------------------------------------------------------
# "cov": by covariate (D groups; covariates without observations are empty groups) | "win": 24-hour windows of the stay |
# "rand": random ids in [-1, 5) with id 2 never used (an empty id) and id -1 present from n = 3 on |
# "inter": n = 200, interleaved groups of 130, 65 and 5 members (blocks of three and two tiles, no contiguous index list) |
# "edges": n = 200, groups of exactly 63, 64 and 65 members, the other 8 observations -1 | "all", "hold": see groups_of
SCHEMES = ["cov", "win", "rand"]
RAND_G = 5


def groups_of(c, p, scheme):
    """(group, ngroups) of patient p of a case (loo_grad_truth.case) in the patient's own (caller) order, from seeds alone"""
    from medgp_amd import crossval
    m, t, y = c["pts"][p]
    n = t.shape[0]
    if scheme == "cov":
        return crossval.by_covariate(m if c["kidx"] == 7 else np.zeros(n, np.int32), c["D"] if c["kidx"] == 7 else 1)
    if scheme == "win":
        return crossval.by_window(t, 24.0)
    if scheme == "all":                         # one group of everything: J is the nlml
        return np.zeros(n, np.int32), 1
    if scheme == "hold":                        # twenty observations held out together, the rest always conditioned on
        return crossval.hold_out(n, np.arange(10, 30))
    g = T._philox(20261208, 1000 * LG.CASE_IDS.index(c["id"]) + p)
    if scheme == "rand":
        ids = g.integers(-1, RAND_G - 1, size=n)
        ids[ids >= 2] += 1                      # id 2 stays empty
        if n >= 3:
            ids[g.integers(0, n)] = -1
        if ids.max() < 0:
            ids[0] = 0
        return ids.astype(np.int32), RAND_G
    assert n == 200
    sizes = {"inter": [130, 65, 5], "edges": [63, 64, 65]}[scheme]
    ids = np.full(n, -1, np.int64)
    ids[g.permutation(n)[:sum(sizes)]] = np.repeat(np.arange(3), sizes)
    return ids.astype(np.int32), 3


# (case id of loo_grad_truth, patient, scheme): the inputs of the GPU tests
def keys():
    out = [("lmc_sizes", p, s) for p in range(7) for s in SCHEMES]
    out += [("lmc_sizes", 6, "inter"), ("lmc_sizes", 6, "edges")]
    out += [("lmc_D24_missing", 0, "cov"), ("lmc_Q9", 0, "cov"), ("sm_Q4", 0, "win"), ("se", 0, "win"), ("lmc_D24_n512", 0, "cov")]
    return out


case = LG.case
_TRUTH, _PROGRAMS = {}, {}


def truth_of(c, p, scheme, jitter_rounds=0):
    """(obj, grad) of patient p of a case under a scheme in long double, computed once per process"""
    key = (c["id"], p, scheme, jitter_rounds)
    if key not in _TRUTH:
        m, t, y = c["pts"][p]
        grp, ng = groups_of(c, p, scheme)
        _TRUTH[key] = lgo_grad(*fam(c), m, t, y, c["th"][p], grp, ng, np.longdouble, jitter_rounds)
    return _TRUTH[key]


def programs_of(c, p, scheme, jitter_rounds=0):
    """dict(truth = (obj, grad), en = [E_b, E_c] (objective), eg = [E_b, E_c] (gradient)) of the two fp64 programs"""
    key = (c["id"], p, scheme, jitter_rounds)
    if key not in _PROGRAMS:
        m, t, y = c["pts"][p]
        grp, ng = groups_of(c, p, scheme)
        tj, tg = truth_of(c, p, scheme, jitter_rounds)
        b = lgo_grad(*fam(c), m, t, y, c["th"][p], grp, ng, np.float64, jitter_rounds)
        cc = lgo_grad_linalg(*fam(c), m, t, y, c["th"][p], grp, ng, jitter_rounds)
        e = [error_pair(b[0], b[1], tj, tg), error_pair(cc[0], cc[1], tj, tg)]
        _PROGRAMS[key] = dict(truth=(tj, tg), en=[x[0] for x in e], eg=[x[1] for x in e])
    return _PROGRAMS[key]


def budget_of(c, p, scheme, jitter_rounds=0):
    """(truth obj, truth grad, objective budget, gradient budget) of patient p of a case under a scheme"""
    r = programs_of(c, p, scheme, jitter_rounds)
    return r["truth"][0], r["truth"][1], min(budget(r["en"], M_OBJ), NLML_BUDGET_CAP), min(budget(r["eg"], M_GRAD), GRAD_BUDGET_CAP)
