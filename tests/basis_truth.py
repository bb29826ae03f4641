"""Extended-precision truth of medgp_basis_nlml_grad / medgp_basis_posterior_batch: fixed effects with a general basis H [n, p], fixed
or integrated out.  y = H beta + f + noise.  Built on nlml_truth.gram with nlml_truth's hand-written factor and triangular inverse and
loo_grad_truth.grad_from_w, independent of oracle/ and of mean_truth.woodbury (which tests/test_basis_truth.py compares it with on the
indicator basis).  With K the matrix that is factored (jitter rounds included), P = K^-1, Lambda = diag(lam), r0 = y - H b0:

    G = L^-1 H,  A = Lambda + G^T G,  w = L^-1 r0,  c = G^T w,  delta = A^-1 c,  beta^ = b0 + delta,  alpha~ = P (y - H beta^)
    MARGINAL  nlml = quad / 2 + log|K| / 2 + log|A| / 2 - sum_{lam_c > 0} log lam_c / 2 + (n - #{lam_c = 0}) log(2 PI) / 2,
              quad = r0^T P r0 - c^T A^-1 c  evaluated as  |w - G delta|^2 + sum lam_c delta_c^2
              W~ = P - P H A^-1 H^T P - alpha~ alpha~^T,   grad_h = tr(W~ dK/dtheta_h) / 2   (noise lines from diag(W~))
              dbeta = d nlml / d b0 = -lam o delta = -H^T alpha~,   beta_cov = A^-1
    FIXED     beta^ = b0, alpha~ = P r0, W~ = P - alpha~ alpha~^T, nlml = |w|^2 / 2 + log|K| / 2 + n log(2 PI) / 2, dbeta = -G^T w = -H^T alpha~,
              beta_cov = 0
    posterior at a point with basis row h*:  V = L^-1 k*,  r = h* - G^T V,  mean = V^T z + r^T beta^,
              var = (k** - V^T V + sigma^2) + r^T A^-1 r   (FIXED: without the last term)

A not positive definite in the working precision (flat-prior columns that are linearly dependent on the patient's rows): status -1, the
failed pivot of its factorisation (a pivot that is NaN or not above 4 p eps A_jj: _chol_or_none); status -1 also for n <= 2 (min_n = 3, the objective's guard;
the posterior takes min_n = 1).

The two legitimate fp64 programs of the budget: (b) `woodbury` in float64; (c) `linalg`: float64 through numpy.linalg on K (inv, solve,
slogdet), A = Lambda + H^T P H and the quadratic form as the DIFFERENCE of the definition.

Error scales: mean_truth's rules for nlml (|nlml| floored at 1e-3 of the largest part), grad, beta and beta_cov (|truth| floored at
1e-3 of the largest of the array); dbeta_c is a sum of terms that cancel (MARGINAL: down to lam_c delta_c, exactly 0 for lam_c = 0):
held on sum_i |H[i, c] alpha~_i|, floored likewise; posterior mean and var on the sum of the absolute values of their terms per point.
"""
import numpy as np

import loo_grad_truth as LG
import mean_truth as MT
import nlml_truth as T
import posterior_jvp_truth as PJ
from mean_truth import FIXED, MARGINAL, error_of, post_errors   # noqa: F401
from nlml_truth import GRAD_BUDGET_CAP, NLML_BUDGET_CAP, U64, budget, spread   # noqa: F401

# ---- the budget (measured by tests/test_basis_truth.py::test_budget_factor_M_and_caps on the CPU programs only, never from device
# output).  M_BASIS = the smallest power of two for which the two fp64 programs (b) and (c) stay within M / 4 times the smaller of
# their errors on every output of every patient of every case, both modes, zero and one jitter round (errors floored at U64).
# Measured: the largest spread is MEASURED_SPREAD (se_p2:2, n = 65, FIXED, the posterior variance; the test prints every output's), so
# M_BASIS / 4 = 32 >= it and 64 / 4 is not.  The effects the cases put into y and the prior means are scaled by 1 / sqrt(p), so that
# H beta stays at the scale of z-scored data: with O(1) coefficients on 64 columns program (c), which takes the quadratic form as a
# difference, loses 85 x the digits of program (b) on the nlml.  The budget of an output of a patient is M_BASIS * max(E_b, E_c, U64); every one stays under NLML_BUDGET_CAP (nlml) /
# GRAD_BUDGET_CAP (everything else) unclipped (the test asserts it).  Provenance: DESIGN.md section 4.7r.
M_BASIS = 128
MEASURED_SPREAD = 29.1
OUTPUTS = ("nlml", "grad", "dbeta", "beta", "beta_cov")


def _chol_or_none(A):
    """column Cholesky with the failure rule of the definition: a pivot that is NaN or not above 4 p eps A_jj (eps of the working
    precision) -- what rounding can leave of a column that is EXACTLY dependent on earlier ones, noise of either sign; 0 for a zero
    column"""
    A = np.array(A)
    n = A.shape[0]
    L = np.zeros_like(A)
    tol = 4 * n * np.finfo(A.dtype).eps
    for j in range(n):
        piv = A[j, j] - L[j, :j] @ L[j, :j]
        if not piv > tol * A[j, j]:
            return None
        L[j, j] = np.sqrt(piv)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def woodbury(kidx, Q, D, R, meta, t, y, theta, H, mode, b0, lam=None, dtype=np.longdouble, jitter_rounds=0, want_grad=True, min_n=3,
             want_parts=False):
    """dict(status, nlml, nlml_mag, grad, dbeta, dbeta_mag, beta, beta_cov [, parts]) in precision dtype; status -1: nothing else"""
    X = dtype
    t32 = np.asarray(t, np.float32)
    n = t32.shape[0]
    Hm = np.asarray(H, np.float64).astype(X).reshape(n, -1)
    p = Hm.shape[1]
    if n < min_n:
        return dict(status=-1)
    yy = np.asarray(y, np.float32).astype(X)
    b0, lam = MT._vec(b0, p, X), MT._vec(lam if mode == MARGINAL else None, p, X)
    K = T.gram(kidx, Q, D, R, meta, t32, theta, X, jitter_rounds)
    L = T._chol_columns(K)
    Li = T._tri_inverse(L)
    z = Li @ yy
    G = Li @ Hm
    w = z - G @ b0
    c = G.T @ w
    logK = np.sum(np.log(np.diagonal(L)))
    log2pi = np.log(2 * X(np.float64(T.REF_PI)))
    if mode == MARGINAL:
        LA = _chol_or_none(np.diag(lam) + G.T @ G)
        if LA is None:
            return dict(status=-1)
        Ti = T._tri_inverse(LA)
        Ainv = Ti.T @ Ti
        delta = Ti.T @ (Ti @ c)
        res = w - G @ delta
        quad = res @ res + np.sum(lam * delta * delta)
        quad_def = (w @ w, c @ (Ainv @ c))
        logA = np.sum(np.log(np.diagonal(LA)))
        pos = lam > 0
        loglam = np.sum(np.log(lam[pos])) / 2
        nfree = int(np.sum(~pos))
        nlml = quad / 2 + logK + logA - loglam + (n - nfree) * log2pi / 2
        parts = [quad_def[0] / 2, quad_def[1] / 2, logK, logA, loglam, (n - nfree) * log2pi / 2]
        dbeta = -(lam * delta)
    else:
        Ti, Ainv, delta = np.zeros((p, p), X), np.zeros((p, p), X), np.zeros(p, X)
        quad = w @ w
        quad_def = (quad, X(0))
        nlml = quad / 2 + logK + n * log2pi / 2
        parts = [quad / 2, logK, n * log2pi / 2]
        dbeta = -c
    beta = b0 + delta
    PH = Li.T @ G
    alpha_t = Li.T @ z - PH @ beta
    out = dict(status=jitter_rounds, nlml=nlml, nlml_mag=max(abs(nlml), X(1e-3) * max(abs(q) for q in parts)), dbeta=dbeta,
               dbeta_mag=np.abs(Hm).T @ np.abs(alpha_t), beta=beta, beta_cov=Ainv, grad=None)
    if want_grad or want_parts:
        Pm = PH @ Ti.T
        W = T._gram_upper_product(Li) - Pm @ Pm.T - np.outer(alpha_t, alpha_t)
        if want_grad:
            out["grad"] = LG.grad_from_w(kidx, Q, D, R, meta, t32, theta, W, X, "blocks")
        if want_parts:
            out["parts"] = dict(L=L, Li=Li, z=z, G=G, Ti=Ti, Ainv=Ainv, W=W, alpha_t=alpha_t, quad=quad, quad_def=quad_def, Hm=Hm)
    return out


def dense(kidx, Q, D, R, meta, t, y, theta, H, b0, lam, dtype=np.longdouble, jitter_rounds=0):
    """MARGINAL with every lam_c > 0 as the zero-mean GP on K~ = K + H Lambda^-1 H^T with data y - H b0"""
    X = dtype
    t32 = np.asarray(t, np.float32)
    n = t32.shape[0]
    Hm = np.asarray(H, np.float64).astype(X).reshape(n, -1)
    b0, lam = MT._vec(b0, Hm.shape[1], X), MT._vec(lam, Hm.shape[1], X)
    assert np.all(lam > 0)
    Kt = T.gram(kidx, Q, D, R, meta, t32, theta, X, jitter_rounds) + (Hm / lam) @ Hm.T
    L = T._chol_columns(Kt)
    Li = T._tri_inverse(L)
    r0 = np.asarray(y, np.float32).astype(X) - Hm @ b0
    z = Li @ r0
    at = Li.T @ z
    nlml = (z @ z) / 2 + np.sum(np.log(np.diagonal(L))) + n * np.log(2 * X(np.float64(T.REF_PI))) / 2
    return dict(nlml=nlml, W=T._gram_upper_product(Li) - np.outer(at, at), alpha_t=at, Li=Li, z=z, Hm=Hm, b0=b0, lam=lam)


def dense_posterior(kidx, Q, D, R, meta, t, y, theta, H, b0, lam, meta2, t2, h2, dtype=np.longdouble, jitter_rounds=0):
    X = dtype
    d = dense(kidx, Q, D, R, meta, t, y, theta, H, b0, lam, X, jitter_rounds)
    Ks, kss, s2 = PJ.cross_gram(kidx, Q, D, R, meta, np.asarray(t, np.float32), theta, meta2, t2, X)
    h2 = np.asarray(h2, np.float64).astype(X).reshape(Ks.shape[1], -1)
    V = d["Li"] @ (Ks + (d["Hm"] / d["lam"]) @ h2.T)
    return h2 @ d["b0"] + V.T @ d["z"], kss + np.sum(h2 * h2 / d["lam"], axis=1) - np.sum(V * V, axis=0) + s2


def posterior(kidx, Q, D, R, meta, t, y, theta, H, mode, b0, lam, meta2, t2, h2, dtype=np.longdouble, jitter_rounds=0):
    """dict(status, mean, var, mag_mean, mag_var, mean0, var0, dmean, extra, beta): mean = mean0 + dmean, var = var0 + extra"""
    X = dtype
    r = woodbury(kidx, Q, D, R, meta, t, y, theta, H, mode, b0, lam, X, jitter_rounds, want_grad=False, min_n=1, want_parts=True)
    if r["status"] < 0:
        return r
    q = r["parts"]
    Ks, kss, s2 = PJ.cross_gram(kidx, Q, D, R, meta, np.asarray(t, np.float32), theta, meta2, t2, X)
    h2 = np.asarray(h2, np.float64).astype(X).reshape(Ks.shape[1], -1)
    V = q["Li"] @ Ks
    rr = h2 - V.T @ q["G"]                       # [m, p]
    mean0, var0 = V.T @ q["z"], kss - np.sum(V * V, axis=0) + s2
    dm = rr @ r["beta"]
    u = rr @ q["Ti"].T
    extra = np.sum(u * u, axis=1)
    mag_mean = np.abs(V).T @ np.abs(q["z"]) + (np.abs(h2) + np.abs(V).T @ np.abs(q["G"])) @ np.abs(r["beta"])
    mag_var = np.abs(kss) + np.sum(V * V, axis=0) + s2 + extra
    return dict(status=r["status"], mean=mean0 + dm, var=var0 + extra, mag_mean=mag_mean, mag_var=mag_var, mean0=mean0, var0=var0,
                dmean=dm, extra=extra, beta=r["beta"])


def linalg(kidx, Q, D, R, meta, t, y, theta, H, mode, b0, lam=None, jitter_rounds=0, points=None):
    """program (c): float64 through numpy.linalg on K; the quadratic form as the difference of the definition.
    points = (meta2, t2, h2): also mean, var"""
    X = np.float64
    t32 = np.asarray(t, np.float32)
    n = t32.shape[0]
    Hm = np.asarray(H, np.float64).reshape(n, -1)
    p = Hm.shape[1]
    yy = np.asarray(y, np.float32).astype(X)
    b0, lam = MT._vec(b0, p, X), MT._vec(lam if mode == MARGINAL else None, p, X)
    K = T.gram(kidx, Q, D, R, meta, t32, theta, X, jitter_rounds)
    P = np.linalg.inv(K)
    P = (P + P.T) / 2
    logK = np.linalg.slogdet(K)[1] / 2
    log2pi = np.log(2 * T.REF_PI)
    r0 = yy - Hm @ b0
    PH = P @ Hm
    if mode == MARGINAL:
        A = np.diag(lam) + Hm.T @ PH
        A = (A + A.T) / 2
        Ainv = np.linalg.inv(A)
        c = PH.T @ r0
        delta = np.linalg.solve(A, c)
        pos = lam > 0
        nlml = (r0 @ (P @ r0) - c @ delta) / 2 + logK + np.linalg.slogdet(A)[1] / 2 - np.sum(np.log(lam[pos])) / 2 + (n - int(np.sum(~pos))) * log2pi / 2
        beta = b0 + delta
        at = P @ (yy - Hm @ beta)
        W = P - PH @ Ainv @ PH.T - np.outer(at, at)
        dbeta = -(Hm.T @ at)
        dbeta[~pos] = 0.0
    else:
        Ainv, beta = np.zeros((p, p)), b0
        at = P @ r0
        nlml = (r0 @ at) / 2 + logK + n * log2pi / 2
        W = P - np.outer(at, at)
        dbeta = -(Hm.T @ at)
    out = dict(status=jitter_rounds, nlml=nlml, grad=LG.grad_from_w(kidx, Q, D, R, meta, t32, theta, W, X, "blocks"), dbeta=dbeta, beta=beta,
               beta_cov=Ainv)
    if points is not None:
        Ks, kss, s2 = PJ.cross_gram(kidx, Q, D, R, meta, t32, theta, points[0], points[1], X)
        rr = np.asarray(points[2], np.float64).reshape(Ks.shape[1], p) - Ks.T @ PH
        out["mean"] = Ks.T @ (P @ yy) + rr @ beta
        out["var"] = kss - np.sum(Ks * (P @ Ks), axis=0) + s2 + np.sum((rr @ Ainv) * rr, axis=1)
    return out


def errors(got, truth):
    """{output: E} of a result dict against the truth dict (outputs the result does not carry are left out)"""
    e = {}
    for k in OUTPUTS:
        if got.get(k) is None or truth.get(k) is None:
            continue
        e[k] = error_of(got[k], truth[k], truth["nlml_mag"] if k == "nlml" else (truth["dbeta_mag"] if k == "dbeta" else None))
    return e


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# (id, kidx, Q, D, R, p, basis kind, [(n, random_patient mode)]): the smallest shapes at which the new kernels can go wrong -- n = 3
# (minimum), 17, 63 / 64 / 65 (block edge), 130 (three 64-row blocks: the triangular k range), 200 (four); p = 1, 2 (one MFMA column
# tile), 16 / 17 (its edge), 33 (the 32-column chunk of the Pm pass), 64 (the capacity edge).  "shuffled" patients arrive with the
# covariates interleaved in time order: the row permutation into the grouped order is not the identity.  Bases:
#   step     one step covering the strict sub-interval [60, 140) of the patient's 200 hours
#   trend    an intercept and a slope in the centred and scaled time (t - 100) / 60 (SE / SM: D = 1)
#   design16 D = 3: intercepts, slopes, harmonics of 24 h and 12 h shared by all covariates, a step [50, 120) and a ramp [30, 90] per
#            covariate (16 columns); design17: beside it a dose column on covariate 1
#   dense    random N(0, 1) entries beside a leading column of ones: well conditioned for n >= 2 p
_SPECS = [
    ("sm_p1", 8, 3, 1, 0, 1, "step", [(17, "plain"), (65, "plain")]),
    ("se_p2", 0, 1, 1, 0, 2, "trend", [(3, "plain"), (64, "plain"), (65, "plain")]),
    ("lmc_D3_p16", 7, 5, 3, 2, 16, "design16", [(63, "shuffled"), (130, "plain"), (200, "shuffled")]),
    ("lmc_D3_p17", 7, 5, 3, 2, 17, "design17", [(65, "shuffled"), (200, "plain")]),
    ("lmc_D24_p33", 7, 5, 24, 8, 33, "dense", [(130, "shuffled"), (64, "plain")]),
    ("lmc_D3_p64", 7, 2, 3, 2, 64, "dense", [(200, "plain"), (130, "shuffled")]),
]
CASE_IDS = [s[0] for s in _SPECS]
# hyper draw of a patient where it is not the first (nlml_truth.DRAWS's rule: a draw whose budget from the CPU programs alone would
# exceed a cap, or on which the two programs are more than M_BASIS / 4 apart, is replaced by the next one, on the CPU)
DRAWS = {("lmc_D24_p33", 0): 1}   # (draw 0: a FIXED gradient budget of 4.8 caps)
LAM_CHOICES = [0.0, 0.05, 1.0, 50.0]   # per column, mixed
COND_FLAT = 1e3                        # a patient whose column-normalised H is worse conditioned draws no flat column
_CASES = {}


def recipe(kind, D):
    """the medgp_amd.basis.Design of a basis kind (None: dense, drawn per patient)"""
    from medgp_amd import basis as B
    if kind == "step":
        return B.Design([B.step(60.0, 140.0)])
    if kind == "trend":
        return B.Design([B.intercept(D), B.linear(D, 100.0, 60.0)])
    if kind in ("design16", "design17"):
        parts = [B.intercept(D), B.linear(D, 100.0, 60.0), B.harmonic(24.0), B.harmonic(12.0)]
        parts += [B.step(50.0, 120.0, [d]) for d in range(D)] + [B.ramp(30.0, 90.0, [d]) for d in range(D)]
        if kind == "design17":
            parts.append(B.dose([20.0, 80.0, 150.0], [1.0, 2.5, 0.5], [1]))
        return B.Design(parts)
    return None


def case(cid):
    """dict(id, kidx, Q, D, R, p, kind, pts, th, H, b0, lam) from seeds alone"""
    if cid not in _CASES:
        from medgp_amd import basis as B
        from medgp_amd import synth
        from random_patients import random_patient
        ci = CASE_IDS.index(cid)
        _, kidx, Q, D, R, p, kind, spec = _SPECS[ci]
        g = T._philox(20261801, ci)
        des = recipe(kind, D)
        pts, th, Hs, b0, lam = [], [], [], [], []
        for q, (n, mode) in enumerate(spec):
            if kidx == 7:
                m, t, y = random_patient(g, D, n, mode)
            else:
                m, t, y = None, np.sort(g.uniform(0.0, 200.0, size=n)).astype(np.float32), g.standard_normal(n).astype(np.float32)
            if des is not None:
                H = des.design(m, t)
            else:
                H = np.concatenate([np.ones((n, 1)), g.standard_normal((n, p - 1))], axis=1)
            assert H.shape == (n, p)
            coef = 0.5 * g.standard_normal(p) / np.sqrt(p)   # the patient's own effects: y carries them, its variance stays O(1)
            y = (y + H @ coef).astype(np.float32)
            pts.append((m, t, y))
            Hs.append(H)
            th.append(synth.theta(4816 + 1000 * DRAWS.get((cid, q), 0), 100 * ci + q, kidx, Q, D, R))
            b0.append(0.5 * g.standard_normal(p) / np.sqrt(p))   # (a prior mean that keeps H b0 at the scale of the data)
            lm = g.choice(LAM_CHOICES, size=p)
            if n < 2 * p or not B.conditioning(H) <= COND_FLAT or np.any(np.sum(H * H, axis=0) == 0):
                lm[lm == 0] = 0.05                           # (these rows do not carry flat coefficients)
            lam.append(lm)
        _CASES[cid] = dict(id=cid, kidx=kidx, Q=Q, D=D, R=R, p=p, kind=kind, pts=pts, th=th, H=Hs, b0=b0, lam=lam)
    return _CASES[cid]


def fam(c):
    return c["kidx"], c["Q"], c["D"], c["R"]


def patients():
    return [(cid, q) for cid in CASE_IDS for q in range(len(case(cid)["pts"]))]


def points(c, q, count=24):
    """(meta2 or None, t2, h2) of patient q from seeds alone: times from 24 h before the first to 24 h after the last observation,
    covariates uniform over all D; h2 from the case's recipe at the points (dense: drawn like H)"""
    ci = CASE_IDS.index(c["id"])
    g = T._philox(20261802, 1000 * ci + q)
    t = c["pts"][q][1]
    t2 = g.uniform(float(t.min()) - 24.0, float(t.max()) + 24.0, size=count).astype(np.float32)
    m2 = g.integers(0, c["D"], size=count).astype(np.int32) if c["kidx"] == 7 else None
    des = recipe(c["kind"], c["D"])
    h2 = des.design(m2, t2) if des is not None else np.concatenate([np.ones((count, 1)), g.standard_normal((count, c["p"] - 1))], axis=1)
    return m2, t2, h2


_PROGRAMS = {}


def programs_for(c, q, mode, H, b0, lam, jitter_rounds=0, pts=None):
    """dict(truth, e = {output: [E_b, E_c]}) of the two fp64 programs on patient q of a case under the basis H and the prior (b0, lam);
    pts = (meta2, t2, h2): also the posterior's mean, var (truth["post"]).  Not cached."""
    m, t, y = c["pts"][q]
    args = (*fam(c), m, t, y, c["th"][q], H, mode, b0, lam)
    tr = woodbury(*args, np.longdouble, jitter_rounds)
    if tr["status"] < 0:
        return dict(truth=tr, e=None)
    b = woodbury(*args, np.float64, jitter_rounds)
    cc = linalg(*args, jitter_rounds, points=pts)
    eb, ec = errors(b, tr), errors(cc, tr)
    if pts is not None:
        tr["post"] = posterior(*args, *pts, np.longdouble, jitter_rounds)
        bp = posterior(*args, *pts, np.float64, jitter_rounds)
        eb.update(post_errors(bp["mean"], bp["var"], tr["post"]))
        ec.update(post_errors(cc["mean"], cc["var"], tr["post"]))
    return dict(truth=tr, e={k: [eb[k], ec[k]] for k in eb})


def cap_of(output):
    return NLML_BUDGET_CAP if output == "nlml" else GRAD_BUDGET_CAP


def budgets(r):
    """{output: budget} of a programs_for / programs_of result (never clipped: test_basis_truth.py asserts every one is under its cap)"""
    return {k: budget(v, M_BASIS) for k, v in r["e"].items()}


def programs_of(c, q, mode, jitter_rounds=0):
    """programs_for on the case's seeded basis, prior and points(c, q), computed once per process"""
    key = (c["id"], q, mode, jitter_rounds)
    if key not in _PROGRAMS:
        _PROGRAMS[key] = programs_for(c, q, mode, c["H"][q], c["b0"][q], c["lam"][q], jitter_rounds, points(c, q))
    return _PROGRAMS[key]


def truth_of(c, q, mode, jitter_rounds=0):
    return programs_of(c, q, mode, jitter_rounds)["truth"]


def budget_of(c, q, mode, jitter_rounds=0):
    """(truth dict, {output: budget}) of patient q of a case; truth status -1: budgets None"""
    r = programs_of(c, q, mode, jitter_rounds)
    if r["e"] is None:
        return r["truth"], None
    return r["truth"], budgets(r)
