"""Extended-precision truth of medgp_hess_vec: products of the exact (observed) Hessian of the data term of the negative log marginal
likelihood with vectors in the hyper space, built on nlml_truth's hyper transforms, Gram matrix, column Cholesky and triangular
inverse, on fisher_truth's Kdot and on loo_grad_truth's W -> g map.  The reference has no such output: this restatement IS the
definition.

    L(theta) = 1/2 y^T K^-1 y + 1/2 log det K + const          (medgp_nlml_grad's objective without the prior stage)
    P = (K + jitter_rounds diag(sigma^2))^-1,  alpha = P y,  W = P - alpha alpha^T,     grad L_h = 1/2 tr(W dK/dtheta_h)
    Kdot = sum_k v_k dK/dtheta_k (fisher_truth.dgram_dir: the UN-jittered K),  beta = P Kdot alpha
    Wdot = -P Kdot P + beta alpha^T + alpha beta^T
    (H v)_h = 1/2 tr(Wdot dK/dtheta_h) + 1/2 tr(W dKdot/dtheta_h)

The first term is loo_grad_truth.grad_from_w(Wdot).  The second needs the second derivatives of the kernel.  With (k, km, kv) =
nlml_truth._sm_factors, w = 2 PI mu, c = 2 (PI v)^2:
    kmm = km - (w dt)^2 k,     kmv = -2 c dt^2 km,     kvv = 2 kv + (2 c dt^2)^2 k
form "naive" (LMC-SM) builds one n x n matrix dKdot/dtheta_h per hyper; form "blocks" takes five block sums of W per component --
S, SM, SV as the gradient and the two raw moments  M3 = sum W e sin(w dt) dt^3,  M4 = sum W e cos(w dt) dt^4  (e = exp(-c dt^2)):
    SMM = SM + (w^2 / 2c) SV,     SMV = 2 c w M3,     SVV = 2 SV + 4 c^2 M4
and the lines of DESIGN.md section 4.7n.  SM and SE have 1 x 1 blocks: one form.  The noise terms are never scaled by 1 + jitter_rounds.

The module also holds the cases shared by tests/test_hess.py and tests/test_hess_gpu.py (those of loo_grad_truth._SPECS with
fisher_truth.directions), the two legitimate fp64 programs the budget is measured on, and the budget constant.
"""
import numpy as np

import fisher_truth as F
import loo_grad_truth as LG
import nlml_truth as T
from fisher_truth import directions   # noqa: F401
from loo_grad_truth import CASE_IDS, COND_MAX, NAIVE_MAX_N, case, cond, fam   # noqa: F401
from nlml_truth import GRAD_BUDGET_CAP, U64, budget, error_pair, spread   # noqa: F401

# ---- the budget (measured by tests/test_hess.py::test_budget_factor_M_and_caps on the CPU programs only) ----
# Two legitimate fp64 programs: (b) this code in float64; (c) P = numpy.linalg.inv(K), alpha = numpy.linalg.solve(K, y), both terms in
# block-sum form.  Starting from the project's M_GRAD = 128: the two programs stay within M / 4 of each other on every case, so the
# starting value stands.  The budget of a case is M_HESS * max(E_b, E_c), floored at M_HESS * U64, capped at GRAD_BUDGET_CAP.  The
# error scale is NOT error_pair's |Hv_h|: a component of H v is the sum of three parts that cancel (scale_of), and on |Hv_h| the CPU
# programs alone exceed the cap (n = 130: 128 * 8.5e-12).  Provenance: DESIGN.md section 4.7n.
M_HESS = 128
NVEC = 2


def _form(n, form):
    return form if form is not None else ("naive" if n <= NAIVE_MAX_N else "blocks")


def _second_factors(h, q, tt, dt):
    """(k, km, kv, kmm, kmv, kvv) of component q"""
    k, km, kv = T._sm_factors(h, q, tt, dt, False)
    w = 2 * h["pi"] * h["mu"][q]
    c = 2 * (h["pi"] * h["v"][q]) ** 2
    r2 = dt * dt
    return k, km, kv, km - (w * w) * r2 * k, -2 * c * r2 * km, 2 * kv + (2 * c * r2) ** 2 * k


def _moments(h, q, tt, dt):
    """(k, km, kv, e sin(w dt) dt^3, e cos(w dt) dt^4, w, c) of component q: what the five block sums are taken against"""
    k, km, kv = T._sm_factors(h, q, tt, dt, False)
    w = 2 * h["pi"] * h["mu"][q]
    c = 2 * (h["pi"] * h["v"][q]) ** 2
    r2 = dt * dt
    e = np.exp(-c * r2)
    return k, km, kv, e * np.sin(w * dt) * dt * r2, e * np.cos(w * dt) * r2 * r2, w, c


def curvature_term(kidx, Q, D, R, meta, t, theta, W, v, dtype=np.longdouble, form="naive"):
    """1/2 tr(W dKdot/dtheta_h) for every hyper, W symmetric, Kdot along v"""
    X = dtype
    h = T.transform(kidx, Q, D, R, theta, X)
    vv = np.asarray(v).astype(X)
    tt = np.asarray(t, np.float32).astype(X)
    n = tt.shape[0]
    dt = tt[:, None] - tt[None, :]
    g = np.zeros(T.num_hyp(kidx, Q, D, R), X)
    wd = np.diagonal(W)
    if kidx == 7:
        m = np.asarray(meta, np.int64)
        E = np.zeros((n, D), X)
        E[np.arange(n), m] = 1
        g[:D] = 2 * h["sig2"] * vv[:D] * (wd @ E)
        cc = vv[D:]
        Ad = cc[:Q * D * R].reshape(Q, D, R)
        vmu, vv_, vk = cc[Q * D * R:Q * D * R + Q], cc[Q * D * R + Q:Q * D * R + 2 * Q], cc[Q * (D * R + 2):].reshape(Q, D)
        o_mu, o_v, o_k = D + Q * D * R, D + Q * D * R + Q, D + Q * (D * R + 2)
        mm = (m[:, None], m[None, :])
        for q in range(Q):
            A, B, kap = h["A"][q], h["B"][q], h["kappa"][q]
            Bd = Ad[q] @ A.T + A @ Ad[q].T
            Bd[np.arange(D), np.arange(D)] += kap * vk[q]
            if form == "naive":
                k, km, kv, kmm, kmv, kvv = _second_factors(h, q, tt, dt)
                mix = vmu[q] * km + vv_[q] * kv
                for d in range(D):
                    for r in range(R):
                        dB, dBd = np.zeros((D, D), X), np.zeros((D, D), X)
                        dB[d, :] += A[:, r]
                        dB[:, d] += A[:, r]
                        dBd[d, :] += Ad[q][:, r]
                        dBd[:, d] += Ad[q][:, r]
                        g[D + q * D * R + d * R + r] = np.sum(W * (dBd[mm] * k + dB[mm] * mix)) / 2
                    sel = ((m == d)[:, None] & (m == d)[None, :]).astype(X)
                    g[o_k + q * D + d] = np.sum(W * sel * kap[d] * (vk[q, d] * k + mix)) / 2
                g[o_mu + q] = np.sum(W * (Bd[mm] * km + B[mm] * (vmu[q] * kmm + vv_[q] * kmv))) / 2
                g[o_v + q] = np.sum(W * (Bd[mm] * kv + B[mm] * (vmu[q] * kmv + vv_[q] * kvv))) / 2
            else:
                k, km, kv, f3, f4, w, c = _moments(h, q, tt, dt)
                S, SM, SV, M3, M4 = (E.T @ ((W * f) @ E) for f in (k, km, kv, f3, f4))
                S, SM, SV, M3, M4 = ((x + x.T) / 2 for x in (S, SM, SV, M3, M4))
                SMM, SMV, SVV = SM + (w * w / (2 * c)) * SV, 2 * c * w * M3, 2 * SV + 4 * c * c * M4
                N = vmu[q] * SM + vv_[q] * SV
                g[D + q * D * R:D + (q + 1) * D * R] = (N @ A + S @ Ad[q]).ravel()
                g[o_mu + q] = (np.sum(Bd * SM) + np.sum(B * (vmu[q] * SMM + vv_[q] * SMV))) / 2
                g[o_v + q] = (np.sum(Bd * SV) + np.sum(B * (vmu[q] * SMV + vv_[q] * SVV))) / 2
                g[o_k + q * D:o_k + (q + 1) * D] = kap * (vk[q] * np.diagonal(S) + np.diagonal(N)) / 2
    elif kidx == 8:
        g[0] = 2 * h["sig2"][0] * vv[0] * np.sum(wd)
        for q in range(Q):
            k, km, kv, f3, f4, w, c = _moments(h, q, tt, dt)
            S, SM, SV, M3, M4 = (np.sum(W * f) for f in (k, km, kv, f3, f4))
            SMM, SMV, SVV = SM + (w * w / (2 * c)) * SV, 2 * c * w * M3, 2 * SV + 4 * c * c * M4
            a, b, cv = vv[1 + q], vv[1 + Q + q], vv[1 + 2 * Q + q]
            wq = h["w"][q]
            g[1 + q] = wq * (a * S + b * SM + cv * SV) / 2
            g[1 + Q + q] = wq * (a * SM + b * SMM + cv * SMV) / 2
            g[1 + 2 * Q + q] = wq * (a * SV + b * SMV + cv * SVV) / 2
    else:
        g[0] = 2 * h["sig2"][0] * vv[0] * np.sum(wd)
        r2 = (dt / h["l"]) ** 2
        e = h["sf2"] * np.exp(-r2 / 2)
        # k_l = e r^2 (= -kv),  k_ll = e (r^4 - 2 r^2) (= kvv),  d/dlog sf = 2
        Sl, Sll, S0 = np.sum(W * e * r2), np.sum(W * e * (r2 * r2 - 2 * r2)), np.sum(W * e)
        g[1] = (vv[1] * Sll + 2 * vv[2] * Sl) / 2
        g[2] = vv[1] * Sl + 2 * vv[2] * S0
    return g


def parts(kidx, Q, D, R, meta, t, y, theta, dtype=np.longdouble, jitter_rounds=0):
    """(P, alpha, W) in precision dtype: column Cholesky, triangular inverse, L^-T L^-1"""
    X = dtype
    t32 = np.asarray(t, np.float32)
    yy = np.asarray(y, np.float32).astype(X)
    K = T.gram(kidx, Q, D, R, meta, t32, theta, X, jitter_rounds)
    Li = T._tri_inverse(T._chol_columns(K))
    P = T._gram_upper_product(Li)
    alpha = Li.T @ (Li @ yy)
    return P, alpha, P - alpha[:, None] * alpha[None, :]


def hess_from_parts(kidx, Q, D, R, meta, t, theta, P, alpha, vecs, dtype=np.longdouble, form=None, want_mag=False):
    """([H v for v in vecs], grad L) from given P and alpha.  H v is the sum of three parts -- the Fisher part 1/2 tr(-P Kdot P dK_h),
    the rank-2 part 1/2 tr((beta alpha^T + alpha beta^T) dK_h) and the curvature part 1/2 tr(W dKdot_h) -- which cancel to a large
    extent; want_mag: also the sum of their magnitudes per direction and hyper, the scale on which H v is known (errors)."""
    X = dtype
    t32 = np.asarray(t, np.float32)
    f = _form(t32.shape[0], form)
    W = P - alpha[:, None] * alpha[None, :]
    W = (W + W.T) / 2
    out, mag = [], []
    for v in np.atleast_2d(np.asarray(vecs)):
        Kd = F.dgram_dir(kidx, Q, D, R, meta, t32, theta, v, X)
        beta = P @ (Kd @ alpha)
        G = P @ Kd @ P
        r2 = beta[:, None] * alpha[None, :] + alpha[:, None] * beta[None, :]
        ga = LG.grad_from_w(kidx, Q, D, R, meta, t32, theta, -(G + G.T) / 2, X, f)
        gb = LG.grad_from_w(kidx, Q, D, R, meta, t32, theta, (r2 + r2.T) / 2, X, f)
        gc = curvature_term(kidx, Q, D, R, meta, t32, theta, W, v, X, f)
        out.append(ga + gb + gc)
        mag.append(np.abs(ga) + np.abs(gb) + np.abs(gc))
    g = LG.grad_from_w(kidx, Q, D, R, meta, t32, theta, W, X, f)
    return (np.array(out), g, np.array(mag)) if want_mag else (np.array(out), g)


def hess_vec(kidx, Q, D, R, meta, t, y, theta, vecs, dtype=np.longdouble, jitter_rounds=0, form=None, want_grad=False, want_mag=False):
    """(grad^2 L)(theta) v for every row v of vecs ([nvec, H] or [H]) in precision dtype: [nvec, H] (and grad L [H], and the
    magnitudes of hess_from_parts)"""
    P, alpha, _ = parts(kidx, Q, D, R, meta, t, y, theta, dtype, jitter_rounds)
    r = hess_from_parts(kidx, Q, D, R, meta, t, theta, P, alpha, vecs, dtype, form, want_mag)
    if want_mag:
        return r if want_grad else (r[0], r[2])
    return r if want_grad else r[0]


def hess_vec_linalg(kidx, Q, D, R, meta, t, y, theta, vecs, jitter_rounds=0):
    """program (c): float64 through numpy.linalg on K (LAPACK's inverse and solve), both terms in block-sum form"""
    t32 = np.asarray(t, np.float32)
    K = T.gram(kidx, Q, D, R, meta, t32, theta, np.float64, jitter_rounds)
    P = np.linalg.inv(K)
    alpha = np.linalg.solve(K, np.asarray(y, np.float32).astype(np.float64))
    return hess_from_parts(kidx, Q, D, R, meta, t, theta, (P + P.T) / 2, alpha, vecs, np.float64, "blocks")[0]


def matvec_of(kidx, Q, D, R, meta, t, y, theta, dtype=np.longdouble, jitter_rounds=0):
    """the truth as the callable medgp_amd.information / curvature take: V [1, nvec, H] -> [1, nvec, H] (float64 in and out)"""
    P, alpha, _ = parts(kidx, Q, D, R, meta, t, y, theta, dtype, jitter_rounds)

    def mv(V):
        V = np.asarray(V, np.float64)
        return np.array([hess_from_parts(kidx, Q, D, R, meta, t, theta, P, alpha, V[0], dtype)[0]]).astype(np.float64)
    return mv


def scale_identity(fam, theta, s, hs, g):
    """s^T H s (+ g_A . vec(A) for LMC-SM, whose A block is not log-parametrised) -- equal to 2 y^T alpha at zero jitter rounds:
    along theta + a s the un-jittered K scales by e^{2a}, so L(a) = e^{-2a} y^T K^-1 y / 2 + n a + const and L'' = 2 y^T alpha, while
    the chain rule gives L'' = s^T H s + g . d^2 theta / d a^2, and d^2 theta / d a^2 = A on the A block, 0 elsewhere."""
    kidx, Q, D, R = fam
    v = np.sum(np.asarray(s).astype(np.longdouble) * np.asarray(hs).astype(np.longdouble))
    if kidx == 7:
        v = v + np.sum(np.asarray(g).astype(np.longdouble)[D:D + Q * D * R] * np.asarray(theta).astype(np.longdouble)[D:D + Q * D * R])
    return v


# ---- the cases -------------------------------------------------------------------------------------------------------------------

_TRUTH, _PROGRAMS = {}, {}


def truth_of(c, p, jitter_rounds=0, nvec=NVEC):
    """([nvec, H], grad [H], magnitudes [nvec, H]) in long double, computed once per process"""
    key = (c["id"], p, jitter_rounds, nvec)
    if key not in _TRUTH:
        m, t, y = c["pts"][p]
        _TRUTH[key] = hess_vec(*fam(c), m, t, y, c["th"][p], directions(c, p, nvec), np.longdouble, jitter_rounds, want_grad=True, want_mag=True)
    return _TRUTH[key]


def scale_of(mag):
    """the error scale of one direction: the magnitude of the three parts of each component, floored at 1e-3 of the largest.  This is
    error_pair's scale with the parts' magnitudes in the place of |H v|: a component of H v is a difference of parts one or two
    orders larger than itself (measured: DESIGN.md section 4.7n), so no fp64 program knows it to a relative error of its own size."""
    mg = np.asarray(mag, np.longdouble)
    return np.maximum(mg, np.longdouble(1e-3) * mg.max())


def errors(got, truth, mag):
    """max_h |got_h - truth_h| / scale_of(mag)_h, worst over the directions; NaN anywhere gives inf"""
    worst = 0.0
    for g, tr, mg in zip(np.asarray(got), truth, mag):
        e = np.abs(np.asarray(g, np.float64).astype(np.longdouble) - tr) / scale_of(mg)
        worst = max(worst, float("inf") if np.isnan(e).any() else float(e.max()))
    return worst


def programs_of(c, p, jitter_rounds=0):
    """dict(truth = [NVEC, H], grad = [H], mag = [NVEC, H], eg = [E_b, E_c]) of the two fp64 programs"""
    key = (c["id"], p, jitter_rounds)
    if key not in _PROGRAMS:
        m, t, y = c["pts"][p]
        tr, tg, mg = truth_of(c, p, jitter_rounds)
        V = directions(c, p)
        b = hess_vec(*fam(c), m, t, y, c["th"][p], V, np.float64, jitter_rounds)
        cc = hess_vec_linalg(*fam(c), m, t, y, c["th"][p], V, jitter_rounds)
        _PROGRAMS[key] = dict(truth=tr, grad=tg, mag=mg, eg=[errors(b, tr, mg), errors(cc, tr, mg)])
    return _PROGRAMS[key]


def budget_of(c, p, jitter_rounds=0):
    """(truth [NVEC, H], magnitudes [NVEC, H], budget) of patient p of a case"""
    r = programs_of(c, p, jitter_rounds)
    return r["truth"], r["mag"], min(budget(r["eg"], M_HESS), GRAD_BUDGET_CAP)
