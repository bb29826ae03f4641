"""Extended-precision truth of medgp_mean_nlml_grad / medgp_mean_posterior_batch: a constant baseline per covariate, fixed or
integrated out.  y = H beta + f + noise, H[i, d] = [m_i = d] (SE / SM: D = 1).  Built on nlml_truth.gram with nlml_truth's hand-written
factor and triangular inverse, independent of oracle/.  With K the matrix that is factored (jitter rounds included), P = K^-1,
Lambda = diag(lam), r0 = y - H b0:

    G = L^-1 H,  A = Lambda + G^T G,  w = L^-1 r0,  c = G^T w,  delta = A^-1 c,  beta^ = b0 + delta,  alpha~ = P (y - H beta^)
    MARGINAL  nlml = (r0^T P r0 - c^T A^-1 c) / 2 + log|K| / 2 + log|A| / 2 - sum_{lam_d > 0} log lam_d / 2 + (n - #{lam_d = 0}) log(2 PI) / 2
              W~ = P - P H A^-1 H^T P - alpha~ alpha~^T,   grad_h = tr(W~ dK/dtheta_h) / 2   (noise lines from diag(W~), never scaled by 1 + k)
              dmean_d = d nlml / d b0_d = -lam_d delta_d = -(H^T alpha~)_d,   beta_cov = A^-1
              d nlml / d lam_d = (A^-1)_dd / 2 + delta_d^2 / 2 - 1 / (2 lam_d)
    FIXED     beta^ = b0, alpha~ = P r0, W~ = P - alpha~ alpha~^T, nlml = r0^T alpha~ / 2 + log|K| / 2 + n log(2 PI) / 2, dmean = -H^T alpha~,
              beta_cov = 0
    posterior at (m*, t*):  V = L^-1 k*,  r = e_{m*} - G^T V,  mean = V^T z + r^T beta^,  var = (k** - V^T V + sigma^2_{m*}) + r^T A^-1 r
              (FIXED: without the last term)

Two forms that must agree (tests/test_mean_truth.py): `woodbury` (the above; the quadratic form evaluated as |w - G delta|^2 +
sum lam delta^2, the minimum of the penalised residual -- in long double it agrees with the difference of the definition to the
rounding of its two terms, which the test checks) and `dense` (all lam_d > 0: the zero-mean formulas on K~ = K + H Lambda^-1 H^T
with data y - H b0).  A covariate without observations under lam_d = 0 is improper: status -1.  status -1 also for n <= 2
(min_n = 3, the objective's guard; the posterior takes min_n = 1).

The two legitimate fp64 programs of the budget: (b) `woodbury` in float64; (c) `linalg`: float64 through numpy.linalg on K
(inv, solve, slogdet), A = Lambda + H^T P H and the quadratic form as the DIFFERENCE of the definition.

Error scales.  grad, beta, beta_cov: error_pair's rule, |truth_h| floored at 1e-3 of the largest of the array (for beta_cov
the floor is 1e-3 / min lam of an unobserved covariate: entries are not known relative to themselves beside 1 / lam).  nlml: a sum of
parts that cancel where lam is small and b0 is far from the data (r0^T P r0 and c^T A^-1 c are then nearly equal), so the same rule
is applied to the parts' magnitudes as hess_truth.scale_of does: |nlml| floored at 1e-3 of the largest part.  dmean_d = -sum_{m_i = d} alpha~_i is a
sum of terms that cancel (in MARGINAL mode down to lam_d delta_d, exactly 0 for lam_d = 0): its scale is sum_{m_i = d} |alpha~_i|,
floored at 1e-3 of the largest -- on |dmean_d| itself program (c), which takes the sum, is up to 500 times further from the truth
than program (b), which takes -lam_d delta_d (measured, tests/test_mean_truth.py prints it).  Posterior mean and
var: the sum of the absolute values of their terms per point, floored at 1e-3 of the largest (posterior_jvp_truth.scale_of).
"""
import numpy as np

import loo_grad_truth as LG
import nlml_truth as T
import posterior_jvp_truth as PJ
from nlml_truth import GRAD_BUDGET_CAP, NLML_BUDGET_CAP, U64, budget, spread   # noqa: F401

MARGINAL, FIXED = 0, 1

# ---- the budget (measured by tests/test_mean_truth.py::test_budget_factor_M_and_caps on the CPU programs only, never from device
# output).  M_MEAN = the smallest power of two for which the two fp64 programs (b) and (c) stay within M / 4 times the smaller of
# their errors on every output of every patient of every case, both modes, zero and one jitter round (errors floored at U64).
# Measured: the largest spread is MEASURED_SPREAD (se, n = 64, FIXED, the gradient; the test prints every output's), so
# M_MEAN / 4 = 32 >= it and 64 / 4 is not.  The budget of an output of a
# patient is M_MEAN * max(E_b, E_c, U64), capped at NLML_BUDGET_CAP (nlml) / GRAD_BUDGET_CAP (everything else).
# Provenance: DESIGN.md section 4.7q.
M_MEAN = 128
MEASURED_SPREAD = 28.7
OUTPUTS = ("nlml", "grad", "dmean", "beta", "beta_cov")


def _meta(kidx, meta, n):
    return np.asarray(meta, np.int64) if kidx == 7 else np.zeros(n, np.int64)


def nout(kidx, D):
    return D if kidx == 7 else 1


def hmat(kidx, D, meta, n, X):
    H = np.zeros((n, nout(kidx, D)), X)
    H[np.arange(n), _meta(kidx, meta, n)] = 1
    return H


def _vec(a, nd, X):
    return np.zeros(nd, X) if a is None else np.asarray(a, np.float64).astype(X).reshape(nd)


def improper(kidx, D, meta, n, mode, lam):
    if mode != MARGINAL:
        return False
    cnt = np.bincount(_meta(kidx, meta, n), minlength=nout(kidx, D))
    return bool(np.any((cnt == 0) & (np.asarray(lam, np.float64) == 0)))


def woodbury(kidx, Q, D, R, meta, t, y, theta, mode, b0, lam=None, dtype=np.longdouble, jitter_rounds=0, want_grad=True, min_n=3,
             want_parts=False):
    """dict(status, nlml, nlml_mag, grad, dmean, beta, beta_cov [, parts]) in precision dtype; status -1: every output None"""
    X = dtype
    t32 = np.asarray(t, np.float32)
    n, nd = t32.shape[0], nout(kidx, D)
    if n < min_n or improper(kidx, D, meta, n, mode, lam):
        return dict(status=-1)
    yy = np.asarray(y, np.float32).astype(X)
    b0, lam = _vec(b0, nd, X), _vec(lam if mode == MARGINAL else None, nd, X)
    Hm = hmat(kidx, D, meta, n, X)
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
        A = np.diag(lam) + G.T @ G
        Ti = T._tri_inverse(T._chol_columns(A))
        Ainv = Ti.T @ Ti
        delta = Ti.T @ (Ti @ c)
        res = w - G @ delta
        quad = res @ res + np.sum(lam * delta * delta)
        quad_def = (w @ w, c @ (Ainv @ c))
        logA = -np.sum(np.log(np.diagonal(Ti)))
        pos = lam > 0
        loglam = np.sum(np.log(lam[pos])) / 2
        nfree = int(np.sum(~pos))
        nlml = quad / 2 + logK + logA - loglam + (n - nfree) * log2pi / 2
        parts = [quad_def[0] / 2, quad_def[1] / 2, logK, logA, loglam, (n - nfree) * log2pi / 2]
        dmean = -(lam * delta)
    else:
        Ti, Ainv, delta = np.zeros((nd, nd), X), np.zeros((nd, nd), X), np.zeros(nd, X)
        quad = w @ w
        quad_def = (quad, X(0))
        nlml = quad / 2 + logK + n * log2pi / 2
        parts = [quad / 2, logK, n * log2pi / 2]
        dmean = -c
    beta = b0 + delta
    PH = Li.T @ G
    alpha_t = Li.T @ z - PH @ beta
    out = dict(status=jitter_rounds, nlml=nlml, nlml_mag=max(abs(nlml), X(1e-3) * max(abs(p) for p in parts)), dmean=dmean,
               dmean_mag=Hm.T @ np.abs(alpha_t), beta=beta, beta_cov=Ainv, grad=None)
    if want_grad or want_parts:
        Pm = PH @ Ti.T
        W = T._gram_upper_product(Li) - Pm @ Pm.T - np.outer(alpha_t, alpha_t)
        if want_grad:
            out["grad"] = LG.grad_from_w(kidx, Q, D, R, meta, t32, theta, W, X, "blocks")
        if want_parts:
            out["parts"] = dict(L=L, Li=Li, z=z, G=G, Ti=Ti, Ainv=Ainv, W=W, alpha_t=alpha_t, quad=quad, quad_def=quad_def, Hm=Hm)
    return out


def dense(kidx, Q, D, R, meta, t, y, theta, b0, lam, dtype=np.longdouble, jitter_rounds=0):
    """MARGINAL with every lam_d > 0 as the zero-mean GP on K~ = K + H Lambda^-1 H^T with data y - H b0:
    dict(nlml, W, alpha_t, Kt_factor pieces) -- what the Woodbury form must agree with"""
    X = dtype
    t32 = np.asarray(t, np.float32)
    n, nd = t32.shape[0], nout(kidx, D)
    b0, lam = _vec(b0, nd, X), _vec(lam, nd, X)
    assert np.all(lam > 0)
    Hm = hmat(kidx, D, meta, n, X)
    Kt = T.gram(kidx, Q, D, R, meta, t32, theta, X, jitter_rounds) + (Hm / lam) @ Hm.T
    L = T._chol_columns(Kt)
    Li = T._tri_inverse(L)
    r0 = np.asarray(y, np.float32).astype(X) - Hm @ b0
    z = Li @ r0
    at = Li.T @ z
    nlml = (z @ z) / 2 + np.sum(np.log(np.diagonal(L))) + n * np.log(2 * X(np.float64(T.REF_PI))) / 2
    return dict(nlml=nlml, W=T._gram_upper_product(Li) - np.outer(at, at), alpha_t=at, Li=Li, z=z, Hm=Hm, b0=b0, lam=lam)


def dense_posterior(kidx, Q, D, R, meta, t, y, theta, b0, lam, meta2, t2, dtype=np.longdouble, jitter_rounds=0):
    X = dtype
    d = dense(kidx, Q, D, R, meta, t, y, theta, b0, lam, X, jitter_rounds)
    Ks, kss, s2 = PJ.cross_gram(kidx, Q, D, R, meta, np.asarray(t, np.float32), theta, meta2, t2, X)
    m2 = _meta(kidx, meta2, Ks.shape[1])
    Kst = Ks + (d["Hm"] / d["lam"])[:, m2]
    V = d["Li"] @ Kst
    return d["b0"][m2] + V.T @ d["z"], kss + 1 / d["lam"][m2] - np.sum(V * V, axis=0) + s2


def posterior(kidx, Q, D, R, meta, t, y, theta, mode, b0, lam, meta2, t2, dtype=np.longdouble, jitter_rounds=0):
    """dict(status, mean, var, mag_mean, mag_var, mean0, var0, dmean, extra): mean = mean0 + dmean, var = var0 + extra"""
    X = dtype
    r = woodbury(kidx, Q, D, R, meta, t, y, theta, mode, b0, lam, X, jitter_rounds, want_grad=False, min_n=1, want_parts=True)
    if r["status"] < 0:
        return r
    p = r["parts"]
    Ks, kss, s2 = PJ.cross_gram(kidx, Q, D, R, meta, np.asarray(t, np.float32), theta, meta2, t2, X)
    mm = Ks.shape[1]
    m2 = _meta(kidx, meta2, mm)
    V = p["Li"] @ Ks
    E2 = np.zeros((mm, nout(kidx, D)), X)
    E2[np.arange(mm), m2] = 1
    rr = E2 - V.T @ p["G"]                       # [m, D]
    mean0, var0 = V.T @ p["z"], kss - np.sum(V * V, axis=0) + s2
    dm = rr @ r["beta"]
    u = rr @ p["Ti"].T
    extra = np.sum(u * u, axis=1)
    mag_mean = np.abs(V).T @ np.abs(p["z"]) + np.abs(rr) @ np.abs(r["beta"])
    mag_var = np.abs(kss) + np.sum(V * V, axis=0) + s2 + extra
    return dict(status=r["status"], mean=mean0 + dm, var=var0 + extra, mag_mean=mag_mean, mag_var=mag_var, mean0=mean0, var0=var0,
                dmean=dm, extra=extra, beta=r["beta"])


def linalg(kidx, Q, D, R, meta, t, y, theta, mode, b0, lam=None, jitter_rounds=0, points=None):
    """program (c): float64 through numpy.linalg on K; the quadratic form as the difference of the definition.  points = (meta2, t2):
    also mean, var"""
    X = np.float64
    t32 = np.asarray(t, np.float32)
    n, nd = t32.shape[0], nout(kidx, D)
    yy = np.asarray(y, np.float32).astype(X)
    b0, lam = _vec(b0, nd, X), _vec(lam if mode == MARGINAL else None, nd, X)
    Hm = hmat(kidx, D, meta, n, X)
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
        dmean = -(Hm.T @ at)
        dmean[~pos] = 0.0
    else:
        Ainv, beta = np.zeros((nd, nd)), b0
        at = P @ r0
        nlml = (r0 @ at) / 2 + logK + n * log2pi / 2
        W = P - np.outer(at, at)
        dmean = -(Hm.T @ at)
    out = dict(status=jitter_rounds, nlml=nlml, grad=LG.grad_from_w(kidx, Q, D, R, meta, t32, theta, W, X, "blocks"), dmean=dmean, beta=beta,
               beta_cov=Ainv)
    if points is not None:
        Ks, kss, s2 = PJ.cross_gram(kidx, Q, D, R, meta, t32, theta, points[0], points[1], X)
        mm = Ks.shape[1]
        E2 = np.zeros((mm, nd))
        E2[np.arange(mm), _meta(kidx, points[0], mm)] = 1
        rr = E2 - Ks.T @ PH
        out["mean"] = Ks.T @ (P @ yy) + rr @ beta
        out["var"] = kss - np.sum(Ks * (P @ Ks), axis=0) + s2 + np.sum((rr @ Ainv) * rr, axis=1)
    return out


def prior_grad(beta, beta_cov, b0, lam):
    """(d nlml / d b0, d nlml / d log lam) of the MARGINAL objective from its outputs (lam_d = 0: both 0 -- the flat prior has no
    parameter); what medgp_amd.baseline.prior_grad restates"""
    X = np.asarray(beta).dtype.type
    b0, lam = np.asarray(b0, np.float64).astype(X), np.asarray(lam, np.float64).astype(X)
    delta = np.asarray(beta) - b0
    dl = np.diagonal(np.asarray(beta_cov)) / 2 + delta * delta / 2
    pos = lam > 0
    return -(lam * delta), np.where(pos, lam * dl - X(0.5), 0)


# ---- errors ------------------------------------------------------------------------------------------------------------------------

def scale_of(mag):
    mg = np.abs(np.asarray(mag, np.longdouble))
    return np.maximum(mg, np.longdouble(1e-3) * mg.max()) if mg.size else mg


def error_of(got, truth, mag=None):
    """max |got - truth| / scale_of(mag or truth); an all-zero scale demands exact zeros; NaN gives inf"""
    got = np.asarray(got, np.float64).astype(np.longdouble).ravel()
    truth = np.asarray(truth, np.longdouble).ravel()
    sc = scale_of(truth if mag is None else np.asarray(mag).ravel())
    assert got.shape == truth.shape == sc.shape, (got.shape, truth.shape, sc.shape)
    if got.size == 0:
        return 0.0
    d = np.abs(got - truth)
    if np.isnan(d).any():
        return float("inf")
    zero = sc == 0
    if zero.any() and d[zero].max() > 0:
        return float("inf")
    return float((d[~zero] / sc[~zero]).max()) if (~zero).any() else 0.0


def errors(got, truth):
    """{output: E} of a result dict against the truth dict (outputs the result does not carry are left out)"""
    e = {}
    for k in OUTPUTS:
        if got.get(k) is None or truth.get(k) is None:
            continue
        e[k] = error_of(got[k], truth[k], truth["nlml_mag"] if k == "nlml" else (truth["dmean_mag"] if k == "dmean" else None))
    return e


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# (id, kidx, Q, D, R, [(n, random_patient mode)]): the smallest shapes at which the new kernels can go wrong -- n = 3 (the n > 2
# guard's edge), 63 / 64 / 65 (block edge), 130 (three blocks: off-diagonal tiles); D = 1 through SM and SE, D = 3, 24, 33 (the Pm panel
# crosses one 32-column chunk), 64 (the full panel); Q = 5 and Q = 9 (two launches of the gradient pass).  "missing" patients have
# covariates without observations, "shuffled" ones arrive with the covariates interleaved.
_SPECS = [
    ("lmc_D3_Q5", 7, 5, 3, 2, [(3, "plain"), (63, "plain"), (64, "shuffled"), (65, "missing"), (130, "plain")]),
    ("lmc_D3_Q9", 7, 9, 3, 2, [(65, "plain"), (130, "shuffled")]),
    ("lmc_D24", 7, 5, 24, 8, [(130, "missing"), (64, "plain")]),
    ("lmc_D33", 7, 2, 33, 2, [(130, "missing"), (65, "shuffled")]),
    ("lmc_D64", 7, 2, 64, 2, [(130, "plain"), (100, "missing")]),
    ("sm_Q3", 8, 3, 1, 0, [(3, "plain"), (65, "plain"), (130, "plain")]),
    ("se", 0, 1, 1, 0, [(64, "plain"), (130, "plain")]),
]
CASE_IDS = [s[0] for s in _SPECS]
# hyper draw of a patient where it is not the first (nlml_truth.DRAWS's rule: a draw whose budget from the CPU programs alone would
# exceed a cap, or on which the two programs are more than M_MEAN / 4 apart, does not belong in the sweep and is replaced by the
# next one, on the CPU: sm_Q3:1 for the gradient cap, lmc_D24:1 for a spread of 38.7 on dmean)
DRAWS = {("sm_Q3", 1): 1, ("lmc_D24", 1): 1}
LAM_CHOICES = [0.0, 0.05, 1.0, 50.0]   # per covariate, mixed; an unobserved covariate never draws 0 (that is the improper entry's test)
_CASES = {}


def case(cid):
    """dict(id, kidx, Q, D, R, pts, th, b0, lam) from seeds alone"""
    if cid not in _CASES:
        from medgp_amd import synth
        from random_patients import random_patient
        ci = CASE_IDS.index(cid)
        _, kidx, Q, D, R, spec = _SPECS[ci]
        g = T._philox(20261701, ci)
        pts, th, b0, lam = [], [], [], []
        for p, (n, mode) in enumerate(spec):
            if kidx == 7:
                m, t, y = random_patient(g, D, n, mode)
            else:
                m, t, y = None, np.sort(g.uniform(0.0, 200.0, size=n)).astype(np.float32), g.standard_normal(n).astype(np.float32)
            nd = nout(kidx, D)
            off = g.standard_normal(nd)                       # the patient's own baselines: y is shifted by them
            y = (y + off[_meta(kidx, m, n)]).astype(np.float32)
            pts.append((m, t, y))
            th.append(synth.theta(4716 + 1000 * DRAWS.get((cid, p), 0), 100 * ci + p, kidx, Q, D, R))
            b0.append(0.5 * g.standard_normal(nd))
            lm = g.choice(LAM_CHOICES, size=nd)
            cnt = np.bincount(_meta(kidx, m, n), minlength=nd)
            lm[(cnt == 0) & (lm == 0)] = 1.0
            if n <= 3:
                lm[lm == 0] = 0.05                            # (three observations do not carry flat baselines)
            lam.append(lm)
        _CASES[cid] = dict(id=cid, kidx=kidx, Q=Q, D=D, R=R, pts=pts, th=th, b0=b0, lam=lam)
    return _CASES[cid]


def fam(c):
    return c["kidx"], c["Q"], c["D"], c["R"]


def patients():
    return [(cid, p) for cid in CASE_IDS for p in range(len(case(cid)["pts"]))]


def points(c, p, count=24):
    """(meta2 or None, t2) of patient p from seeds alone: times from 24 h before the first to 24 h after the last observation,
    covariates uniform over all D (unobserved ones included)"""
    ci = CASE_IDS.index(c["id"])
    g = T._philox(20261702, 1000 * ci + p)
    t = c["pts"][p][1]
    t2 = g.uniform(float(t.min()) - 24.0, float(t.max()) + 24.0, size=count).astype(np.float32)
    m2 = g.integers(0, c["D"], size=count).astype(np.int32) if c["kidx"] == 7 else None
    return m2, t2


_PROGRAMS = {}


def truth_of(c, p, mode, jitter_rounds=0):
    """the long-double result dict (with grad, and "post": mean / var / mags at points(c, p)), computed once per process"""
    return programs_of(c, p, mode, jitter_rounds)["truth"]


def post_errors(mean, var, post):
    return dict(mean=error_of(mean, post["mean"], post["mag_mean"]), var=error_of(var, post["var"], post["mag_var"]))


def programs_for(c, p, mode, b0, lam, jitter_rounds=0, pts=None):
    """dict(truth, e = {output: [E_b, E_c]}) of the two fp64 programs on patient p of a case under ANOTHER baseline (b0, lam) than
    the seeded one; pts = (meta2, t2): also the posterior's mean, var (truth["post"]).  Not cached."""
    m, t, y = c["pts"][p]
    args = (*fam(c), m, t, y, c["th"][p], mode, b0, lam)
    tr = woodbury(*args, np.longdouble, jitter_rounds)
    if tr["status"] < 0:
        return dict(truth=tr, e=None)
    b = woodbury(*args, np.float64, jitter_rounds)
    cc = linalg(*args, jitter_rounds, points=pts)
    eb, ec = errors(b, tr), errors(cc, tr)
    if pts is not None:
        tr["post"] = posterior(*args, pts[0], pts[1], np.longdouble, jitter_rounds)
        bp = posterior(*args, pts[0], pts[1], np.float64, jitter_rounds)
        eb.update(post_errors(bp["mean"], bp["var"], tr["post"]))
        ec.update(post_errors(cc["mean"], cc["var"], tr["post"]))
    return dict(truth=tr, e={k: [eb[k], ec[k]] for k in eb})


def budgets(r):
    """{output: budget} of a programs_for / programs_of result, capped"""
    return {k: min(budget(v, M_MEAN), cap_of(k)) for k, v in r["e"].items()}


def programs_of(c, p, mode, jitter_rounds=0):
    """programs_for on the case's seeded baseline and points(c, p), computed once per process"""
    key = (c["id"], p, mode, jitter_rounds)
    if key not in _PROGRAMS:
        _PROGRAMS[key] = programs_for(c, p, mode, c["b0"][p], c["lam"][p], jitter_rounds, points(c, p))
    return _PROGRAMS[key]


def cap_of(output):
    return NLML_BUDGET_CAP if output == "nlml" else GRAD_BUDGET_CAP


def budget_of(c, p, mode, jitter_rounds=0):
    """(truth dict, {output: budget}) of patient p of a case; truth status -1: budgets None"""
    r = programs_of(c, p, mode, jitter_rounds)
    if r["e"] is None:
        return r["truth"], None
    return r["truth"], budgets(r)
