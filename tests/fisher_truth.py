"""Extended-precision truth of medgp_fisher_vec: products of the Fisher information of the Gaussian marginal likelihood with vectors
in the hyper space, built on nlml_truth's hyper transforms, Gram matrix, column Cholesky and triangular inverse and on
loo_grad_truth's W -> g map.  The reference has no such output: this restatement IS the definition.

    F_hk = 1/2 tr(P dK/dtheta_h P dK/dtheta_k),     P = (K + jitter_rounds diag(sigma^2))^-1
    Kdot = sum_k v_k dK/dtheta_k                    (dgram_dir: the derivative of the UN-jittered K along v)
    (F v)_h = 1/2 tr(W dK/dtheta_h),     W = sym(P Kdot P)     (loo_grad_truth.grad_from_w)

For LMC-SM, v = [v_sigma | Adot | v_mu | v_v | v_kappa] in theta order and (k, km, kv) = nlml_truth._sm_factors:
    Bdot_q = Adot_q A_q^T + A_q Adot_q^T + diag(kappa_q o v_kappa,q)
    Kdot_ij = sum_q (Bdot_q[m_i,m_j] k_q + B_q[m_i,m_j] (v_mu,q km_q + v_v,q kv_q))(t_i - t_j) + delta_ij 2 sigma^2_{m_i} v_sigma,m_i
SM: w_q (v_w,q k_q + v_mu,q km_q + v_v,q kv_q);  SE: v_l e r^2 + 2 v_sf e with e = sf^2 exp(-r^2 / 2), r = dt / l.
The noise term is not scaled by 1 + jitter_rounds.  F does not depend on y and has no prior part.  form: "naive" up to
loo_grad_truth.NAIVE_MAX_N observations, "blocks" above (as the LOO truth).

The module also holds the cases shared by tests/test_fisher.py (CPU: the budget conditions) and tests/test_fisher_gpu.py (the device
held to the budget) -- those of loo_grad_truth._SPECS with the same seeds for patients and theta, directions standard normals from
_philox --, the two legitimate fp64 programs the budget is measured on, and the budget constant.
"""
import numpy as np

import loo_grad_truth as LG
import nlml_truth as T
from loo_grad_truth import CASE_IDS, COND_MAX, NAIVE_MAX_N, case, cond, fam   # noqa: F401
from nlml_truth import GRAD_BUDGET_CAP, U64, budget, error_pair, spread   # noqa: F401

# ---- the budget (measured by tests/test_fisher.py::test_budget_factor_M_and_caps on the CPU programs only) ----
# Two legitimate fp64 programs: (b) this code in float64; (c) P = numpy.linalg.inv(K), the gradient in block-sum form.  Starting from the
# project's M_GRAD = 128: the two programs stay within M / 4 of each other on every case, so the starting value stands.  The budget of
# a case is M_FISHER * max(E_b, E_c), floored at M_FISHER * U64, capped at GRAD_BUDGET_CAP.  Provenance: DESIGN.md section 4.7m.
M_FISHER = 128
NVEC = 2                   # directions per patient the budget tests use


def dgram_dir(kidx, Q, D, R, meta, t, theta, v, dtype=np.longdouble):
    """Kdot = sum_k v_k dK/dtheta_k of the un-jittered K, in precision dtype"""
    X = dtype
    h = T.transform(kidx, Q, D, R, theta, X)
    vv = np.asarray(v).astype(X)          # (a long-double direction is taken as it is: test_fisher.py's difference quotients)
    assert vv.shape == (T.num_hyp(kidx, Q, D, R),), vv.shape
    tt = np.asarray(t, np.float32).astype(X)
    n = tt.shape[0]
    m = np.asarray(meta, np.int64) if kidx == 7 else np.zeros(n, np.int64)
    dt = tt[:, None] - tt[None, :]
    Kd = np.zeros((n, n), X)
    if kidx == 7:
        c = vv[D:]
        Ad = c[:Q * D * R].reshape(Q, D, R)
        vmu, vv_, vk = c[Q * D * R:Q * D * R + Q], c[Q * D * R + Q:Q * D * R + 2 * Q], c[Q * (D * R + 2):].reshape(Q, D)
        for q in range(Q):
            k, km, kv = T._sm_factors(h, q, tt, dt, False)
            Bd = Ad[q] @ h["A"][q].T + h["A"][q] @ Ad[q].T
            Bd[np.arange(D), np.arange(D)] += h["kappa"][q] * vk[q]
            Kd += Bd[m[:, None], m[None, :]] * k + h["B"][q][m[:, None], m[None, :]] * (vmu[q] * km + vv_[q] * kv)
    elif kidx == 8:
        for q in range(Q):
            k, km, kv = T._sm_factors(h, q, tt, dt, False)
            Kd += h["w"][q] * (vv[1 + q] * k + vv[1 + Q + q] * km + vv[1 + 2 * Q + q] * kv)
    else:
        r2 = (dt / h["l"]) ** 2
        e = h["sf2"] * np.exp(-r2 / 2)
        Kd += vv[1] * e * r2 + 2 * vv[2] * e
    nl = D if kidx == 7 else 1
    Kd[np.arange(n), np.arange(n)] += 2 * h["sig2"][m] * vv[:nl][m]
    return Kd


def inverse(kidx, Q, D, R, meta, t, theta, dtype=np.longdouble, jitter_rounds=0):
    """P = (K + jitter_rounds diag(sigma^2))^-1: column Cholesky, triangular inverse, L^-T L^-1"""
    K = T.gram(kidx, Q, D, R, meta, np.asarray(t, np.float32), theta, dtype, jitter_rounds)
    return T._gram_upper_product(T._tri_inverse(T._chol_columns(K)))


def _form(n, form):
    return form if form is not None else ("naive" if n <= NAIVE_MAX_N else "blocks")


def fisher_from_inverse(kidx, Q, D, R, meta, t, theta, P, vecs, dtype=np.longdouble, form=None):
    """[F v for v in vecs] from a given P"""
    t32 = np.asarray(t, np.float32)
    f = _form(t32.shape[0], form)
    out = []
    for v in np.atleast_2d(np.asarray(vecs, np.float64)):
        W = P @ dgram_dir(kidx, Q, D, R, meta, t32, theta, v, dtype) @ P
        out.append(LG.grad_from_w(kidx, Q, D, R, meta, t32, theta, (W + W.T) / 2, dtype, f))
    return np.array(out)


def fisher_vec(kidx, Q, D, R, meta, t, theta, vecs, dtype=np.longdouble, jitter_rounds=0, form=None):
    """F(theta) v for every row v of vecs ([nvec, H] or [H]) in precision dtype: [nvec, H].  y plays no part."""
    P = inverse(kidx, Q, D, R, meta, t, theta, dtype, jitter_rounds)
    return fisher_from_inverse(kidx, Q, D, R, meta, t, theta, P, vecs, dtype, form)


def fisher_vec_linalg(kidx, Q, D, R, meta, t, theta, vecs, jitter_rounds=0):
    """program (c): float64 through numpy.linalg.inv on K, the gradient in block-sum form"""
    K = T.gram(kidx, Q, D, R, meta, np.asarray(t, np.float32), theta, np.float64, jitter_rounds)
    P = np.linalg.inv(K)
    return fisher_from_inverse(kidx, Q, D, R, meta, t, theta, (P + P.T) / 2, vecs, np.float64, "blocks")


def matvec_of(kidx, Q, D, R, meta, t, theta, dtype=np.longdouble, jitter_rounds=0):
    """the truth as the callable medgp_amd.information takes: V [1, nvec, H] -> [1, nvec, H] (float64 in and out)"""
    P = inverse(kidx, Q, D, R, meta, t, theta, dtype, jitter_rounds)

    def mv(V):
        V = np.asarray(V, np.float64)
        return np.array([fisher_from_inverse(kidx, Q, D, R, meta, t, theta, P, V[0], dtype)]).astype(np.float64)
    return mv


# ---- the cases -------------------------------------------------------------------------------------------------------------------

def directions(c, p, nvec=NVEC):
    """nvec standard-normal directions of patient p of a case, from seeds alone; direction j does not depend on nvec"""
    ci = CASE_IDS.index(c["id"])
    H = T.num_hyp(*fam(c))
    return np.array([T._philox(20261301, 1000 * ci + 10 * p + j).standard_normal(H) for j in range(nvec)])


_TRUTH, _PROGRAMS = {}, {}


def truth_of(c, p, jitter_rounds=0, nvec=NVEC):
    """[nvec, H] in long double, computed once per process"""
    key = (c["id"], p, jitter_rounds, nvec)
    if key not in _TRUTH:
        m, t, _ = c["pts"][p]
        _TRUTH[key] = fisher_vec(*fam(c), m, t, c["th"][p], directions(c, p, nvec), np.longdouble, jitter_rounds)
    return _TRUTH[key]


def errors(got, truth):
    """the gradient error of error_pair, worst over the directions"""
    return max(error_pair(1.0, g, 1.0, tr)[1] for g, tr in zip(np.asarray(got), truth))


def programs_of(c, p, jitter_rounds=0):
    """dict(truth = [NVEC, H], eg = [E_b, E_c]) of the two fp64 programs"""
    key = (c["id"], p, jitter_rounds)
    if key not in _PROGRAMS:
        m, t, _ = c["pts"][p]
        tr = truth_of(c, p, jitter_rounds)
        V = directions(c, p)
        b = fisher_vec(*fam(c), m, t, c["th"][p], V, np.float64, jitter_rounds)
        cc = fisher_vec_linalg(*fam(c), m, t, c["th"][p], V, jitter_rounds)
        _PROGRAMS[key] = dict(truth=tr, eg=[errors(b, tr), errors(cc, tr)])
    return _PROGRAMS[key]


def budget_of(c, p, jitter_rounds=0):
    """(truth [NVEC, H], budget) of patient p of a case"""
    r = programs_of(c, p, jitter_rounds)
    return r["truth"], min(budget(r["eg"], M_FISHER), GRAD_BUDGET_CAP)
