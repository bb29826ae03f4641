"""Extended-precision truth of medgp_hetero_nlml_grad / medgp_hetero_posterior_batch / medgp_robust_nlml_grad: per-observation noise
scales and Student-t robust training.  Built on nlml_truth.gram with nlml_truth's hand-written factor and triangular inverse and
loo_grad_truth.grad_from_w, independent of oracle/.  Row i has covariate d = m_i (SE / SM: D = 1), scale s_i > 0 and, with r jitter
rounds, the factored noise N_i = (1 + r) sigma^2_d s_i (a jitter round adds the SCALED noise vector again).  K_s = K + diag(N),
P = K_s^-1, alpha = P y:

    nlml = y^T alpha / 2 + log|K_s| / 2 + n log(2 PI) / 2,      grad_h = tr((P - alpha alpha^T) dK_s / dtheta_h) / 2
    the noise hyper of covariate d: sigma^2_d sum_{m_i = d} s_i W_ii -- nlml_truth's noise line with s_i W_ii in the place of W_ii
    (like it NOT scaled by 1 + r: the reference's quirk the device follows)
    resid_i = y_i - E f_i = N_i alpha_i,    fvar_i = var f_i = N_i - N_i^2 P_ii
    posterior at (m*, t*), V = L^-1 k*:  mean = V^T z,  var = k** - V^T V + sigma^2_{m*} s2        (s2: per point, None = 1, 0 = latent)

status -1: n < min_n (3 for the objectives, 1 for the posterior).

Student-t noise as a Gaussian scale mixture, eps_i | tau_i ~ N(0, sigma^2_d / tau_i), tau_i ~ Gamma(nu_d / 2, nu_d / 2), with
q(tau_i) = Gamma(a_d, a_d s_i), a_d = (nu_d + 1) / 2 (E tau_i = 1 / s_i) and q(f) optimal for s: the negative evidence bound is

    J(theta, nu, s) = nlml(theta; s) + sum_i kappa(nu_{m_i}, s_i),   kappa(nu, s) = C(nu) + c (log s + 1 / s),   c = nu / 2
    C(nu) = psi(a) / 2 - lgamma(a) + lgamma(c) + c log(a / c) - a - (psi(a) - log a) / 2

(-E log N(eps; 0, sigma^2 / tau) against the Gaussian term at precision 1 / (sigma^2 s) leaves -(psi(a) - log a) / 2 per row; the
rest is KL(q(tau) || p(tau))).  J >= the exact Student-t nlml, and at fixed s dJ / dtheta is the heteroscedastic gradient exactly.
One E-step from a factorisation at s:  e_i = (resid_i^2 + fvar_i) / sigma^2_{m_i},  s_i <- (nu_d + e_i) / (nu_d + 1).  `robust` takes
s0, makes `sweeps` E-steps and evaluates J, its gradient, resid and fvar at the last scales; delta = max_i |s_new - s_old| / s_new of
the last E-step (0 without one).

The two legitimate fp64 programs of the budget: (b) the same code in float64 (psi and lgamma from scipy.special); (c) `linalg`:
float64 through numpy.linalg on K_s (inv, slogdet) with fvar written as N (1 - N P_ii) and C(nu) in its reduced form (the psi terms
cancel).

Error scales.  nlml and grad: mean_truth's / error_pair's rules.  resid: |N_i alpha_i|.  fvar: N_i + N_i^2 P_ii.  scale: the chain
through e_i, (nu + (2 resid_i^2 + N_i + N_i^2 P_ii) / sigma^2) / (nu + 1).  delta: (scale's magnitude + |s_old|) / s_new at its
largest.  J: nlml's rule plus the sum of the absolute values of the terms of kappa.  mean: sum_i |V_i z_i|; var: |k**| + V^T V +
sigma^2 s2.  Each floored at 1e-3 of the largest of its array.
"""
import math

import numpy as np

import loo_grad_truth as LG
import nlml_truth as T
import posterior_jvp_truth as PJ
from mean_truth import error_of, scale_of   # noqa: F401
from nlml_truth import GRAD_BUDGET_CAP, NLML_BUDGET_CAP, U64, budget, spread   # noqa: F401

# ---- the budget (measured by tests/test_hetero_truth.py::test_budget_factor_M_and_caps on the CPU programs only, never from device
# output).  M_HET = the smallest power of two for which the two fp64 programs (b) and (c) stay within M / 4 times the smaller of
# their errors on every output of every patient of every case, with zero and one jitter round and 0, 1 and 5 sweeps (errors floored at
# U64).  MEASURED_SPREAD is the largest spread the test printed.  The budget of an output of a patient is M_HET * max(E_b, E_c, U64);
# the case set keeps every one under NLML_BUDGET_CAP (nlml, obj) / GRAD_BUDGET_CAP (everything else) unclipped.
M_HET = 128
MEASURED_SPREAD = 22.1
SWEEPS = (0, 1, 5)
OBJ_OUTPUTS = ("nlml", "grad", "resid", "fvar")
POST_OUTPUTS = ("mean", "var")
ROB_OUTPUTS = ("obj", "grad", "scale", "delta", "resid", "fvar")
X = np.longdouble


def _meta(kidx, meta, n):
    return np.asarray(meta, np.int64) if kidx == 7 else np.zeros(n, np.int64)


def nout(kidx, D):
    return D if kidx == 7 else 1


def _special(x, dtype):
    """(psi(x), lgamma(x)) in precision dtype: mpmath at 40 digits for the long double, scipy.special for float64"""
    if dtype is np.float64:
        from scipy.special import digamma, gammaln
        return np.float64(digamma(float(x))), np.float64(gammaln(float(x)))
    import mpmath
    with mpmath.workdps(40):
        v = mpmath.mpf(float(x))
        return X(mpmath.nstr(mpmath.digamma(v), 30)), X(mpmath.nstr(mpmath.loggamma(v), 30))


def kappa_const(nu, dtype=np.longdouble, reduced=False):
    """(C(nu), the sum of the absolute values of its terms) in precision dtype; reduced: without the two psi terms that cancel"""
    Xd = dtype
    nu = Xd(np.float64(nu))
    c, a = nu / 2, (nu + 1) / 2
    psi, lga = _special(np.float64(a), Xd)
    lgc = _special(np.float64(c), Xd)[1]
    if reduced:
        terms = [-lga, lgc, c * np.log(a / c), -a, np.log(a) / 2]
    else:
        terms = [psi / 2, -lga, lgc, c * np.log(a / c), -a, -(psi - np.log(a)) / 2]
    tot = Xd(0)
    for v in terms:
        tot = tot + v
    return tot, sum(abs(v) for v in terms)


def hetero(kidx, Q, D, R, meta, t, y, theta, scale, dtype=np.longdouble, jitter_rounds=0, want_grad=True, min_n=3, want_parts=False):
    """dict(status, nlml, nlml_mag, grad, resid, fvar, fvar_mag, N, pdiag, sig2 [, parts]) in precision dtype; status -1: no outputs"""
    Xd = dtype
    t32 = np.asarray(t, np.float32)
    n = t32.shape[0]
    if n < min_n:
        return dict(status=-1)
    m = _meta(kidx, meta, n)
    h = T.transform(kidx, Q, D, R, theta, Xd)
    s = np.asarray(scale, np.float64).astype(Xd)
    assert s.shape == (n,)
    N = (1 + jitter_rounds) * (h["sig2"][m] * s)
    K = T.gram(kidx, Q, D, R, meta, t32, theta, Xd, -1)          # (1 + (-1)) sigma^2 = no noise: K alone
    K[np.arange(n), np.arange(n)] += N
    yy = np.asarray(y, np.float32).astype(Xd)
    L = T._chol_columns(K)
    Li = T._tri_inverse(L)
    z = Li @ yy
    alpha = Li.T @ z
    logK = np.sum(np.log(np.diagonal(L)))
    log2pi = np.log(2 * Xd(np.float64(T.REF_PI)))
    parts = [(yy @ alpha) / 2, logK, n * log2pi / 2]
    nlml = parts[0] + parts[1] + parts[2]
    P = T._gram_upper_product(Li)
    pd = np.diagonal(P).copy()
    out = dict(status=jitter_rounds, nlml=nlml, nlml_mag=max(abs(nlml), Xd(1e-3) * max(abs(p) for p in parts)), grad=None,
               resid=N * alpha, fvar=N - N * N * pd, fvar_mag=N + N * N * pd, N=N, pdiag=pd, sig2=h["sig2"][m])
    if want_grad:
        W = P - np.outer(alpha, alpha)
        g = LG.grad_from_w(kidx, Q, D, R, meta, t32, theta, W, Xd, "blocks")
        wd = np.diagonal(W) * s
        for d in range(nout(kidx, D)):
            g[d] = h["sig2"][d] * np.sum(wd[m == d])
        out["grad"] = g
    if want_parts:
        out["parts"] = dict(Li=Li, z=z, alpha=alpha)
    return out


def posterior(kidx, Q, D, R, meta, t, y, theta, scale, meta2, t2, s2=None, dtype=np.longdouble, jitter_rounds=0):
    """dict(status, mean, var, mag_mean, mag_var) in precision dtype"""
    Xd = dtype
    r = hetero(kidx, Q, D, R, meta, t, y, theta, scale, Xd, jitter_rounds, want_grad=False, min_n=1, want_parts=True)
    p = r["parts"]
    Ks, kss, sg = PJ.cross_gram(kidx, Q, D, R, meta, np.asarray(t, np.float32), theta, meta2, t2, Xd)
    if s2 is not None:
        sg = sg * np.asarray(s2, np.float64).astype(Xd)
    V = p["Li"] @ Ks
    vv = np.sum(V * V, axis=0)
    return dict(status=r["status"], mean=V.T @ p["z"], var=kss - vv + sg, mag_mean=np.abs(V).T @ np.abs(p["z"]), mag_var=np.abs(kss) + vv + sg)


def _nu_rows(kidx, D, nu, m, Xd):
    return np.asarray(nu, np.float64).reshape(nout(kidx, D)).astype(Xd)[m]


def estep(r, nu_rows):
    """(the new scales, their error magnitude) from the result dict of `hetero`"""
    e = (r["resid"] ** 2 + r["fvar"]) / r["sig2"]
    emag = (2 * r["resid"] ** 2 + r["fvar_mag"]) / r["sig2"]
    return (nu_rows + e) / (nu_rows + 1), (nu_rows + emag) / (nu_rows + 1)


def robust(kidx, Q, D, R, meta, t, y, theta, nu, sweeps, scale0=None, dtype=np.longdouble, jitter_rounds=0, want_grad=True):
    """dict(status, obj, obj_mag, grad, scale, scale_mag, delta, delta_mag, resid, fvar, fvar_mag, trace = [J after 0, 1, .. sweeps])"""
    Xd = dtype
    n = np.asarray(t).shape[0]
    if n < 3:
        return dict(status=-1)
    m = _meta(kidx, meta, n)
    nur = _nu_rows(kidx, D, nu, m, Xd)
    s = np.ones(n, Xd) if scale0 is None else np.asarray(scale0, np.float64).astype(Xd)
    smag = np.abs(s)
    delta, dmag = Xd(0), Xd(0)
    cst = [kappa_const(v, Xd) for v in np.asarray(nu, np.float64).reshape(-1)]

    def bound(r, s):
        c = nur / 2
        k = np.sum(c * (np.log(s) + 1 / s)) + sum(cst[d][0] for d in m)
        kmag = np.sum(c * (np.abs(np.log(s)) + 1 / s)) + sum(cst[d][1] for d in m)
        return r["nlml"] + k, r["nlml_mag"] + kmag

    trace = []
    for _ in range(sweeps):
        r = hetero(kidx, Q, D, R, meta, t, y, theta, s, Xd, jitter_rounds, want_grad=False)
        trace.append(bound(r, s)[0])
        sn, snmag = estep(r, nur)
        rel = np.abs(sn - s) / sn
        i = int(np.argmax(rel))
        delta, dmag = rel[i], np.max((snmag + smag) / sn)
        s, smag = sn, snmag
    r = hetero(kidx, Q, D, R, meta, t, y, theta, s, Xd, jitter_rounds, want_grad=want_grad)
    obj, omag = bound(r, s)
    trace.append(obj)
    return dict(status=r["status"], obj=obj, obj_mag=omag, grad=r["grad"], scale=s, scale_mag=smag, delta=delta, delta_mag=dmag,
                resid=r["resid"], fvar=r["fvar"], fvar_mag=r["fvar_mag"], trace=trace)


# ---- program (c): numpy.linalg ------------------------------------------------------------------------------------------------

def linalg(kidx, Q, D, R, meta, t, y, theta, scale, jitter_rounds=0, points=None, want_grad=True):
    """float64 through numpy.linalg on K_s, fvar as N (1 - N P_ii).  points = (meta2, t2, s2): also the posterior's outputs"""
    Xd = np.float64
    t32 = np.asarray(t, np.float32)
    n = t32.shape[0]
    m = _meta(kidx, meta, n)
    h = T.transform(kidx, Q, D, R, theta, Xd)
    s = np.asarray(scale, np.float64)
    N = (1 + jitter_rounds) * (h["sig2"][m] * s)
    K = T.gram(kidx, Q, D, R, meta, t32, theta, Xd, -1)
    K[np.arange(n), np.arange(n)] += N
    yy = np.asarray(y, np.float32).astype(Xd)
    P = np.linalg.inv(K)
    P = (P + P.T) / 2
    alpha = P @ yy
    pd = np.diagonal(P).copy()
    out = dict(status=jitter_rounds, nlml=(yy @ alpha) / 2 + np.linalg.slogdet(K)[1] / 2 + n * np.log(2 * T.REF_PI) / 2, resid=N * alpha,
               fvar=N * (1 - N * pd), sig2=h["sig2"][m], grad=None)
    if want_grad:
        W = P - np.outer(alpha, alpha)
        g = LG.grad_from_w(kidx, Q, D, R, meta, t32, theta, W, Xd, "blocks")
        wd = np.diagonal(W) * s
        for d in range(nout(kidx, D)):
            g[d] = h["sig2"][d] * np.sum(wd[m == d])
        out["grad"] = g
    if points is not None:
        meta2, t2, s2 = points
        Ks, kss, sg = PJ.cross_gram(kidx, Q, D, R, meta, t32, theta, meta2, t2, Xd)
        if s2 is not None:
            sg = sg * np.asarray(s2, np.float64)
        out["mean"] = Ks.T @ alpha
        out["var"] = kss - np.sum(Ks * (P @ Ks), axis=0) + sg
    return out


def robust_linalg(kidx, Q, D, R, meta, t, y, theta, nu, sweeps, scale0=None, jitter_rounds=0):
    n = np.asarray(t).shape[0]
    m = _meta(kidx, meta, n)
    nur = _nu_rows(kidx, D, nu, m, np.float64)
    s = np.ones(n) if scale0 is None else np.asarray(scale0, np.float64).copy()
    delta = 0.0
    for _ in range(sweeps):
        r = linalg(kidx, Q, D, R, meta, t, y, theta, s, jitter_rounds, want_grad=False)
        sn = (nur + (r["resid"] ** 2 + r["fvar"]) / r["sig2"]) / (nur + 1)
        delta = np.max(np.abs(sn - s) / sn)
        s = sn
    r = linalg(kidx, Q, D, R, meta, t, y, theta, s, jitter_rounds)
    cst = [kappa_const(v, np.float64, reduced=True)[0] for v in np.asarray(nu, np.float64).reshape(-1)]
    k = np.sum((nur / 2) * (np.log(s) + 1 / s)) + math.fsum(cst[d] for d in m)
    return dict(status=r["status"], obj=r["nlml"] + k, grad=r["grad"], scale=s, delta=delta, resid=r["resid"], fvar=r["fvar"])


# ---- errors ------------------------------------------------------------------------------------------------------------------------

def errors(got, truth):
    """{output: E} of the objective outputs a result dict carries against the truth dict of `hetero`"""
    mags = {"nlml": truth["nlml_mag"], "fvar": truth["fvar_mag"]}
    return {k: error_of(got[k], truth[k], mags.get(k)) for k in OBJ_OUTPUTS if got.get(k) is not None and truth.get(k) is not None}


def post_errors(got, post):
    return {k: error_of(got[k], post[k], post["mag_" + k]) for k in POST_OUTPUTS if got.get(k) is not None}


def robust_errors(got, truth):
    mags = {"obj": truth["obj_mag"], "fvar": truth["fvar_mag"], "scale": truth["scale_mag"], "delta": truth["delta_mag"]}
    return {k: error_of(got[k], truth[k], mags.get(k)) for k in ROB_OUTPUTS if got.get(k) is not None and truth.get(k) is not None}


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# (id, kidx, Q, D, R, [(n, random_patient mode)]): the smallest shapes at which the kernels can go wrong -- n = 3 (the n > 2 guard's
# edge), 64 / 65 (the 64-row block edge), 130 in an ungrouped caller order (three blocks, a second size class, the look-ahead route),
# SE at n = 64, SM (Q = 3) at n = 100, Q = 9 at n = 70 (the two-pass assembly).  Scales log-uniform in [1/8, 8] on every row (grouped
# rows 0, 63, 64 and the last among them); nu per covariate in [2, 8]; y = a sample of the heteroscedastic model with two rows moved
# by six noise standard deviations.
_SPECS = [
    ("lmc_D3_Q5", 7, 5, 3, 2, [(3, "plain"), (64, "shuffled"), (65, "shuffled"), (130, "shuffled")]),
    ("se", 0, 1, 1, 0, [(64, "plain")]),
    ("sm_Q3", 8, 3, 1, 0, [(100, "plain")]),
    ("lmc_Q9", 7, 9, 3, 2, [(70, "shuffled")]),
]
CASE_IDS = [s[0] for s in _SPECS]
JITTER_CASE, JITTER_PS = "lmc_D3_Q5", [1, 2, 3]      # the patients the one-jitter-round test runs
# hyper draw of a patient where it is not the first (nlml_truth.DRAWS's rule, decided on the CPU programs alone)
DRAWS = {}
_CASES = {}


def case(cid):
    """dict(id, kidx, Q, D, R, pts, th, scale, nu) from seeds alone"""
    if cid not in _CASES:
        from medgp_amd import synth
        from random_patients import random_patient
        ci = CASE_IDS.index(cid)
        _, kidx, Q, D, R, spec = _SPECS[ci]
        g = T._philox(20262101, ci)
        nd = nout(kidx, D)
        pts, th, scs, nus = [], [], [], []
        for p, (n, mode) in enumerate(spec):
            if kidx == 7:
                m, t, _ = random_patient(g, D, n, mode)
            else:
                m, t = None, np.sort(g.uniform(0.0, 200.0, size=n)).astype(np.float32)
            theta = synth.theta(5016 + 1000 * DRAWS.get((cid, p), 0), 100 * ci + p, kidx, Q, D, R)
            s = np.exp(g.uniform(np.log(0.125), np.log(8.0), size=n))
            mm = _meta(kidx, m, n)
            sig2 = np.asarray(T.transform(kidx, Q, D, R, theta, np.float64)["sig2"])[mm]
            K = T.gram(kidx, Q, D, R, m, t, theta, np.float64, -1)
            K[np.arange(n), np.arange(n)] += sig2 * s
            y = np.linalg.cholesky(K) @ g.standard_normal(n)
            out = g.choice(n, size=min(2, n), replace=False)
            y[out] += 6.0 * np.sqrt(sig2[out]) * np.where(g.uniform(size=out.shape[0]) < 0.5, -1.0, 1.0)
            pts.append((m, t, y.astype(np.float32)))
            th.append(theta)
            scs.append(s)
            nus.append(g.uniform(2.0, 8.0, size=nd))
        _CASES[cid] = dict(id=cid, kidx=kidx, Q=Q, D=D, R=R, pts=pts, th=th, scale=scs, nu=nus)
    return _CASES[cid]


def fam(c):
    return c["kidx"], c["Q"], c["D"], c["R"]


def patients():
    return [(cid, p) for cid in CASE_IDS for p in range(len(case(cid)["pts"]))]


def points(c, p, count=12):
    """(meta2 or None, t2, s2) of patient p from seeds alone: times from 24 h before the first to 24 h after the last observation,
    covariates uniform over all D, s2 log-uniform in [1/8, 8] with the first two points at 0 (the latent f) and 1"""
    ci = CASE_IDS.index(c["id"])
    g = T._philox(20262102, 1000 * ci + p)
    t = c["pts"][p][1]
    t2 = g.uniform(float(t.min()) - 24.0, float(t.max()) + 24.0, size=count).astype(np.float32)
    m2 = g.integers(0, c["D"], size=count).astype(np.int32) if c["kidx"] == 7 else None
    s2 = np.exp(g.uniform(np.log(0.125), np.log(8.0), size=count))
    s2[:2] = (0.0, 1.0)
    return m2, t2, s2


_PROGRAMS = {}


def programs_for(c, p, scale, jitter_rounds=0, pts=None, nu=None, sweeps=()):
    """dict(truth, e = {output: [E_b, E_c]}) of the two fp64 programs on patient p of a case under the scales `scale`; pts = (meta2,
    t2, s2): also the posterior's outputs (truth["post"]); nu with sweeps: also the robust call's from ones, keyed r<sweeps>_<output>
    (truth["rob"][sweeps]).  Not cached."""
    m, t, y = c["pts"][p]
    args = (*fam(c), m, t, y, c["th"][p])
    tr = hetero(*args, scale, np.longdouble, jitter_rounds)
    if tr["status"] < 0:
        return dict(truth=tr, e=None)
    b = hetero(*args, scale, np.float64, jitter_rounds)
    cc = linalg(*args, scale, jitter_rounds, points=pts)
    eb, ec = errors(b, tr), errors(cc, tr)
    if pts is not None:
        tr["post"] = posterior(*args, scale, *pts, np.longdouble, jitter_rounds)
        bp = posterior(*args, scale, *pts, np.float64, jitter_rounds)
        eb.update(post_errors(bp, tr["post"]))
        ec.update(post_errors(cc, tr["post"]))
    tr["rob"] = {}
    for k in sweeps:
        rt = robust(*args, nu, k, None, np.longdouble, jitter_rounds)
        rb = robust(*args, nu, k, None, np.float64, jitter_rounds)
        rc = robust_linalg(*args, nu, k, None, jitter_rounds)
        tr["rob"][k] = rt
        eb.update({f"r{k}_{o}": v for o, v in robust_errors(rb, rt).items()})
        ec.update({f"r{k}_{o}": v for o, v in robust_errors(rc, rt).items()})
    return dict(truth=tr, e={k: [eb[k], ec[k]] for k in eb})


def cap_of(output):
    return NLML_BUDGET_CAP if output.split("_")[-1] in ("nlml", "obj") else GRAD_BUDGET_CAP


def budgets(r):
    """{output: budget} of a programs_for / programs_of result (never clipped: test_hetero_truth.py asserts every one under its cap)"""
    return {k: budget(v, M_HET) for k, v in r["e"].items()}


def programs_of(c, p, jitter_rounds=0):
    """programs_for on the case's seeded scales, points and nu with every sweep count of SWEEPS, computed once per process"""
    key = (c["id"], p, jitter_rounds)
    if key not in _PROGRAMS:
        _PROGRAMS[key] = programs_for(c, p, c["scale"][p], jitter_rounds, points(c, p), c["nu"][p], SWEEPS)
    return _PROGRAMS[key]


def truth_of(c, p, jitter_rounds=0):
    return programs_of(c, p, jitter_rounds)["truth"]


def budget_of(c, p, jitter_rounds=0):
    """(truth dict, {output: budget}) of patient p of a case; truth status -1: budgets None"""
    r = programs_of(c, p, jitter_rounds)
    if r["e"] is None:
        return r["truth"], None
    return r["truth"], budgets(r)
