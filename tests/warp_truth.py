"""Extended-precision truth of medgp_warp_nlml_grad / medgp_warp_posterior_batch: a warped GP with the sinh-arcsinh map per covariate.
Built on nlml_truth.gram with nlml_truth's hand-written factor and triangular inverse and loo_grad_truth.grad_from_w, independent of
oracle/.  For observation i of covariate d = m_i (SE / SM: D = 1), psi_d = (a, eps, lambda), delta = exp(lambda), s = asinh(y_i),
u = delta s - eps:

    z_i = a + sinh(u),   log g'_i = lambda + log cosh(u) - log(1 + y_i^2) / 2,   g^-1(z) = sinh((asinh(z - a) + eps) / delta)
    dz_i / d(a, eps, lambda) = (1, -cosh u, delta s cosh u),   dlog g'_i / d(a, eps, lambda) = (0, -tanh u, 1 + delta s tanh u)

kind[d] = NONE: z = y exactly, log g' = 0, dpsi = 0.  With K the matrix that is factored (jitter rounds included), P = K^-1,
w = L^-1 z, alpha~ = P z:

    nlml = |w|^2 / 2 + log|K| / 2 + n log(2 PI) / 2 - sum_i log g'_i,   grad_h = tr((P - alpha~ alpha~^T) dK/dtheta_h) / 2
    dpsi[d][k] = sum_{m_i = d} (alpha~_i dz_i/dpsi_k - dlog g'_i/dpsi_k),   logjac = sum_i log g'_i
    posterior at (m*, t*), V = L^-1 k*:  zmean = V^T w,  zvar = k** - V^T V + sigma^2_{m*},  quant_k = g^-1(zmean + zq_k sqrt(zvar)),
    lpd = -log(2 PI zvar) / 2 - (g(y2) - zmean)^2 / (2 zvar) + log g'(y2)

status -1: n < min_n (3 for the objective, 1 for the posterior) or a warped observation that is not finite.

The two legitimate fp64 programs of the budget: (b) `objective` / `posterior` in float64; (c) `linalg`: float64 through numpy.linalg on
K (inv, slogdet) with the warp written differently -- sinh and cosh through exp, log cosh through logaddexp.

Error scales.  grad: error_pair's rule, |truth_h| floored at 1e-3 of the largest.  nlml: |nlml| floored at 1e-3 of its largest part
(mean_truth's rule).  logjac: the sum over i of the absolute values of the three terms of log g'_i (at psi = 0 the terms cancel to
0).  dpsi[d][k] is a sum of terms that cancel: sum_{m_i = d} (|alpha~_i dz_i| + |dlog g'_i|), floored at 1e-3 of the largest of the array.
zmean: sum_i |V_i w_i|; zvar: |k**| + V^T V + sigma^2; lpd: the sum of
the absolute values of its terms, |log(2 PI zvar)| / 2 + r^2 / (2 zvar) + the three terms of log g'(y2), with r = g(y2) - zmean; quant:
max(|quant|, (dg^-1/dz) (|zmean| + |zq| sd)) -- the inverse map amplifies an error in z by its slope.  Each floored at 1e-3 of the
largest of its array.
"""
import numpy as np

import loo_grad_truth as LG
import nlml_truth as T
import posterior_jvp_truth as PJ
from mean_truth import error_of, scale_of   # noqa: F401
from nlml_truth import GRAD_BUDGET_CAP, NLML_BUDGET_CAP, U64, budget, spread   # noqa: F401

NONE, SAS = 0, 1

# ---- the budget (measured by tests/test_warp_truth.py::test_budget_factor_M_and_caps on the CPU programs only, never from device
# output).  M_WARP = the smallest power of two for which the two fp64 programs (b) and (c) stay within M / 4 times the smaller of
# their errors on every output of every patient of every case, zero and one jitter round (errors floored at U64).  Measured: the
# largest spread is MEASURED_SPREAD (se, n = 64, the gradient; the test prints every output's), so M_WARP / 4 = 16 >= it and 32 / 4
# is not.  The budget of an
# output of a patient is M_WARP * max(E_b, E_c, U64); the case set keeps every one under NLML_BUDGET_CAP (nlml) / GRAD_BUDGET_CAP
# (everything else) unclipped.  Provenance: DESIGN.md section 4.7s.
M_WARP = 64
MEASURED_SPREAD = 12.7
# how far medgp_amd.warp.moments at 32 nodes lies from a dense quadrature over the case set, relative to the predictive sd in
# observation space: (mean, sd) worst case, and the same with the points of delta < 0.75 left out (the worst point has delta >= 0.75,
# so the two coincide: the predictive sd in z is at most 1.02 over the set, see medgp_amd/warp.py).  Recorded, not a bar.
MOMENTS_MEASURED = dict(all=(2.2e-7, 3.1e-7), delta_ge_075=(2.2e-7, 3.1e-7))
OBJ_OUTPUTS = ("nlml", "grad", "dpsi", "logjac")
POST_OUTPUTS = ("zmean", "zvar", "quant", "lpd")


def _meta(kidx, meta, n):
    return np.asarray(meta, np.int64) if kidx == 7 else np.zeros(n, np.int64)


def nout(kidx, D):
    return D if kidx == 7 else 1


def _kind(kind, nd):
    return np.full(nd, SAS, np.int64) if kind is None else np.asarray(kind, np.int64).reshape(nd)


def warp(y, m, psi, kind, X, style="direct"):
    """(z, log g', dz [n, 3], dlog g' [n, 3], the sum of the absolute values of the three terms of log g') of values y on covariates m
    in precision X.  style "exp": sinh and cosh through exp and log cosh through logaddexp (program (c))."""
    nd = np.asarray(psi).size // 3
    ps = np.asarray(psi, np.float64).astype(X).reshape(nd, 3)
    sas = (_kind(kind, nd) == SAS)[m]
    yy = np.asarray(y).astype(X)
    a, e, lam = ps[m, 0], ps[m, 1], ps[m, 2]
    dl = np.exp(lam)
    s = np.arcsinh(yy)
    u = dl * s - e
    with np.errstate(over="ignore", invalid="ignore"):
        if style == "exp":
            ep, em = np.exp(u), np.exp(-u)
            sh, ch = (ep - em) / 2, (ep + em) / 2
            lch = np.logaddexp(u, -u) - np.log(X(2))
            th = sh / ch
        else:
            sh, ch, th = np.sinh(u), np.cosh(u), np.tanh(u)
            au = np.abs(u)
            lch = au + np.log1p(np.exp(-2 * au)) - np.log(X(2))
        z = np.where(sas, a + sh, yy)
        lj = np.where(sas, lam + lch - np.log1p(yy * yy) / 2, X(0))
        one, zero = np.ones_like(yy), np.zeros_like(yy)
        dz = np.where(sas[:, None], np.stack([one, -ch, dl * s * ch], axis=1), X(0))
        dlj = np.where(sas[:, None], np.stack([zero, -th, 1 + dl * s * th], axis=1), X(0))
        ljmag = np.where(sas, np.abs(lam) + np.abs(lch) + np.log1p(yy * yy) / 2, X(0))
    return z, lj, dz, dlj, ljmag


def inverse(z, m, psi, kind, X):
    """(g^-1(z), dg^-1/dz) on covariates m"""
    nd = np.asarray(psi).size // 3
    ps = np.asarray(psi, np.float64).astype(X).reshape(nd, 3)
    sas = (_kind(kind, nd) == SAS)[m]
    a, e, dl = ps[m, 0], ps[m, 1], np.exp(ps[m, 2])
    v = (np.arcsinh(z - a) + e) / dl
    return np.where(sas, np.sinh(v), z), np.where(sas, np.cosh(v) / (dl * np.sqrt(1 + (z - a) ** 2)), X(1))


def objective(kidx, Q, D, R, meta, t, y, theta, psi, kind=None, dtype=np.longdouble, jitter_rounds=0, want_grad=True, min_n=3,
              want_parts=False):
    """dict(status, nlml, nlml_mag, grad, dpsi [D, 3], dpsi_mag, logjac, logjac_mag [, parts]) in precision dtype; status -1: no outputs"""
    X = dtype
    t32 = np.asarray(t, np.float32)
    n, nd = t32.shape[0], nout(kidx, D)
    if n < min_n:
        return dict(status=-1)
    m = _meta(kidx, meta, n)
    z, lj, dz, dlj, ljmag = warp(np.asarray(y, np.float32), m, psi, kind, X)
    if not np.all(np.isfinite(z)):
        return dict(status=-1)
    K = T.gram(kidx, Q, D, R, meta, t32, theta, X, jitter_rounds)
    L = T._chol_columns(K)
    Li = T._tri_inverse(L)
    w = Li @ z
    at = Li.T @ w
    logK = np.sum(np.log(np.diagonal(L)))
    log2pi = np.log(2 * X(np.float64(T.REF_PI)))
    logjac = np.sum(lj)
    quad = w @ w
    nlml = quad / 2 + logK + n * log2pi / 2 - logjac
    parts = [quad / 2, logK, n * log2pi / 2, logjac]
    E = np.zeros((n, nd), X)
    E[np.arange(n), m] = 1
    terms = at[:, None] * dz - dlj
    out = dict(status=jitter_rounds, nlml=nlml, nlml_mag=max(abs(nlml), X(1e-3) * max(abs(p) for p in parts)), logjac=logjac,
               logjac_mag=np.sum(ljmag), dpsi=E.T @ terms, dpsi_mag=E.T @ (np.abs(at[:, None] * dz) + np.abs(dlj)), grad=None)
    if want_grad:
        W = T._gram_upper_product(Li) - np.outer(at, at)
        out["grad"] = LG.grad_from_w(kidx, Q, D, R, meta, t32, theta, W, X, "blocks")
    if want_parts:
        out["parts"] = dict(Li=Li, w=w, at=at, z=z, lj=lj)
    return out


def posterior(kidx, Q, D, R, meta, t, y, theta, psi, kind, meta2, t2, y2, zq, dtype=np.longdouble, jitter_rounds=0):
    """dict(status, zmean, zvar, quant [m, nq], lpd (None without y2), mag_*) in precision dtype"""
    X = dtype
    r = objective(kidx, Q, D, R, meta, t, y, theta, psi, kind, X, jitter_rounds, want_grad=False, min_n=1, want_parts=True)
    if r["status"] < 0:
        return r
    p = r["parts"]
    Ks, kss, s2 = PJ.cross_gram(kidx, Q, D, R, meta, np.asarray(t, np.float32), theta, meta2, t2, X)
    mm = Ks.shape[1]
    m2 = _meta(kidx, meta2, mm)
    V = p["Li"] @ Ks
    zmean, vv = V.T @ p["w"], np.sum(V * V, axis=0)
    zvar = kss - vv + s2
    mag_zmean, mag_zvar = np.abs(V).T @ np.abs(p["w"]), np.abs(kss) + vv + s2
    sd = np.sqrt(zvar)
    zqx = np.asarray(zq, np.float64).astype(X)
    zt = zmean[:, None] + zqx[None, :] * sd[:, None]
    mq = np.repeat(m2[:, None], zqx.shape[0], axis=1)
    quant, slope = inverse(zt, mq, psi, kind, X)
    mag_quant = np.maximum(np.abs(quant), slope * (np.abs(zmean)[:, None] + np.abs(zqx)[None, :] * sd[:, None]))
    out = dict(status=r["status"], zmean=zmean, zvar=zvar, quant=quant, lpd=None, mag_zmean=mag_zmean, mag_zvar=mag_zvar, mag_quant=mag_quant,
               mag_lpd=None)
    if y2 is not None:
        gy, lj, _, _, ljmag = warp(np.asarray(y2, np.float32), m2, psi, kind, X)
        log2pi = np.log(2 * X(np.float64(T.REF_PI)))
        res = gy - zmean
        out["lpd"] = -(log2pi + np.log(zvar)) / 2 - res * res / (2 * zvar) + lj
        out["mag_lpd"] = np.abs(log2pi + np.log(zvar)) / 2 + res * res / (2 * zvar) + ljmag
    return out


def linalg(kidx, Q, D, R, meta, t, y, theta, psi, kind=None, jitter_rounds=0, points=None):
    """program (c): float64 through numpy.linalg on K, the warp through exp / logaddexp.  points = (meta2, t2, y2, zq): also the
    posterior's outputs"""
    X = np.float64
    t32 = np.asarray(t, np.float32)
    n, nd = t32.shape[0], nout(kidx, D)
    m = _meta(kidx, meta, n)
    z, lj, dz, dlj, _ = warp(np.asarray(y, np.float32), m, psi, kind, X, "exp")
    K = T.gram(kidx, Q, D, R, meta, t32, theta, X, jitter_rounds)
    P = np.linalg.inv(K)
    P = (P + P.T) / 2
    at = P @ z
    logjac = np.sum(lj)
    nlml = (z @ at) / 2 + np.linalg.slogdet(K)[1] / 2 + n * np.log(2 * T.REF_PI) / 2 - logjac
    W = P - np.outer(at, at)
    E = np.zeros((n, nd))
    E[np.arange(n), m] = 1
    out = dict(status=jitter_rounds, nlml=nlml, logjac=logjac, dpsi=E.T @ (at[:, None] * dz - dlj),
               grad=LG.grad_from_w(kidx, Q, D, R, meta, t32, theta, W, X, "blocks"))
    if points is not None:
        meta2, t2, y2, zq = points
        Ks, kss, s2 = PJ.cross_gram(kidx, Q, D, R, meta, t32, theta, meta2, t2, X)
        m2 = _meta(kidx, meta2, Ks.shape[1])
        out["zmean"] = Ks.T @ at
        out["zvar"] = kss - np.sum(Ks * (P @ Ks), axis=0) + s2
        sd = np.sqrt(out["zvar"])
        zqx = np.asarray(zq, np.float64)
        zt = out["zmean"][:, None] + zqx[None, :] * sd[:, None]
        ps = np.asarray(psi, np.float64).reshape(nd, 3)
        sas = (_kind(kind, nd) == SAS)[m2][:, None]
        v = (np.arcsinh(zt - ps[m2, 0][:, None]) + ps[m2, 1][:, None]) / np.exp(ps[m2, 2])[:, None]
        out["quant"] = np.where(sas, (np.exp(v) - np.exp(-v)) / 2, zt)
        gy, l2, _, _, _ = warp(np.asarray(y2, np.float32), m2, psi, kind, X, "exp")
        res = gy - out["zmean"]
        out["lpd"] = -np.log(2 * T.REF_PI * out["zvar"]) / 2 - res * res / (2 * out["zvar"]) + l2
    return out


# ---- errors ------------------------------------------------------------------------------------------------------------------------

def errors(got, truth):
    """{output: E} of a result dict against the truth dict of `objective` (outputs the result does not carry are left out)"""
    e = {}
    for k in OBJ_OUTPUTS:
        if got.get(k) is None or truth.get(k) is None:
            continue
        mag = {"nlml": truth["nlml_mag"], "logjac": truth["logjac_mag"], "dpsi": truth["dpsi_mag"]}.get(k)
        e[k] = error_of(got[k], truth[k], mag)
    return e


def post_errors(got, post):
    """{output: E} of the posterior outputs a result dict carries against the truth dict of `posterior`"""
    return {k: error_of(got[k], post[k], post["mag_" + k]) for k in POST_OUTPUTS if got.get(k) is not None and post.get(k) is not None}


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# (id, kidx, Q, D, R, kind, nq, [(n, random_patient mode)]): the smallest shapes at which the new kernels can go wrong -- n = 3 (the
# n > 2 guard's edge), 17, 63 / 64 / 65 (the 64-row panel edge), 130 (two size classes beside the small ones; above 128 the look-ahead
# route and the second 128-column block of k_warp_solve), 200; D = 1 through SE and SM, 3, 24.  "shuffled" patients arrive with the
# covariates interleaved, "missing" ones have covariates without observations.  lmc_D3_mixed: kind mixes NONE and SAS.  Patient
# lmc_D3_Q5:1 has psi = 0.  y = g^-1(a sample of the GP + noise): the model is well specified.  nq = 1 (the median), 3, 64.
_SPECS = [
    ("se", 0, 1, 1, 0, None, 1, [(3, "plain"), (64, "plain"), (130, "plain")]),
    ("sm_Q3", 8, 3, 1, 0, None, 3, [(17, "plain"), (65, "plain"), (200, "plain")]),
    ("lmc_D3_Q5", 7, 5, 3, 2, None, 64, [(3, "plain"), (63, "shuffled"), (64, "shuffled"), (65, "missing"), (130, "shuffled"), (200, "shuffled")]),
    ("lmc_D3_mixed", 7, 2, 3, 2, [SAS, NONE, SAS], 3, [(65, "shuffled"), (130, "plain")]),
    ("lmc_D24", 7, 5, 24, 8, None, 64, [(130, "missing"), (64, "shuffled"), (200, "shuffled")]),
]
CASE_IDS = [s[0] for s in _SPECS]
ZERO_PSI = ("lmc_D3_Q5", 1)
JITTER_CASE, JITTER_PS = "lmc_D3_Q5", [1, 2, 3, 4]      # the patients the one-jitter-round test runs
# hyper draw of a patient where it is not the first (nlml_truth.DRAWS's rule: a draw whose budget from the CPU programs alone would
# exceed a cap, or on which the two programs are more than M_WARP / 4 apart, is replaced by the next one, on the CPU)
DRAWS = {("se", 2): 1}   # (draw 0: a spread of 77.1 on lpd, whose budget would be 1.2 caps at any M that covers it)
ZQ = {1: np.zeros(1), 3: np.array([-1.959963984540054, 0.0, 1.959963984540054]), 64: np.linspace(-3.0, 3.0, 64)}
_CASES = {}


def case(cid):
    """dict(id, kidx, Q, D, R, kind, nq, zq, pts, th, psi) from seeds alone"""
    if cid not in _CASES:
        from medgp_amd import synth
        from random_patients import random_patient
        ci = CASE_IDS.index(cid)
        _, kidx, Q, D, R, kind, nq, spec = _SPECS[ci]
        g = T._philox(20261901, ci)
        nd = nout(kidx, D)
        pts, th, psis = [], [], []
        for p, (n, mode) in enumerate(spec):
            if kidx == 7:
                m, t, _ = random_patient(g, D, n, mode)
            else:
                m, t = None, np.sort(g.uniform(0.0, 200.0, size=n)).astype(np.float32)
            theta = synth.theta(4916 + 1000 * DRAWS.get((cid, p), 0), 100 * ci + p, kidx, Q, D, R)
            psi = np.stack([g.uniform(-0.5, 0.5, nd), g.uniform(-1.0, 1.0, nd), g.uniform(-0.7, 0.7, nd)], axis=1)
            if (cid, p) == ZERO_PSI:
                psi = np.zeros((nd, 3))
            K = T.gram(kidx, Q, D, R, m, t, theta, np.float64)
            zs = np.linalg.cholesky(K) @ g.standard_normal(n)
            y = inverse(zs, _meta(kidx, m, n), psi, kind, np.float64)[0].astype(np.float32)
            pts.append((m, t, y))
            th.append(theta)
            psis.append(psi)
        _CASES[cid] = dict(id=cid, kidx=kidx, Q=Q, D=D, R=R, kind=None if kind is None else np.asarray(kind, np.int32), nq=nq, zq=ZQ[nq],
                           pts=pts, th=th, psi=psis)
    return _CASES[cid]


def fam(c):
    return c["kidx"], c["Q"], c["D"], c["R"]


def patients():
    return [(cid, p) for cid in CASE_IDS for p in range(len(case(cid)["pts"]))]


def points(c, p, count=24):
    """(meta2 or None, t2, y2) of patient p from seeds alone: times from 24 h before the first to 24 h after the last observation
    (between and beyond the observations), covariates uniform over all D (unobserved ones included), y2 = g^-1(N(0, 1.5^2))"""
    ci = CASE_IDS.index(c["id"])
    g = T._philox(20261902, 1000 * ci + p)
    t = c["pts"][p][1]
    t2 = g.uniform(float(t.min()) - 24.0, float(t.max()) + 24.0, size=count).astype(np.float32)
    m2 = g.integers(0, c["D"], size=count).astype(np.int32) if c["kidx"] == 7 else None
    y2 = inverse(1.5 * g.standard_normal(count), _meta(c["kidx"], m2, count), c["psi"][p], c["kind"], np.float64)[0].astype(np.float32)
    return m2, t2, y2


_PROGRAMS = {}


def programs_for(c, p, psi, kind, jitter_rounds=0, pts=None, zq=None):
    """dict(truth, e = {output: [E_b, E_c]}) of the two fp64 programs on patient p of a case under the warp (psi, kind); pts =
    (meta2, t2, y2) with zq: also the posterior's outputs (truth["post"]).  Not cached."""
    m, t, y = c["pts"][p]
    args = (*fam(c), m, t, y, c["th"][p], psi, kind)
    tr = objective(*args, np.longdouble, jitter_rounds)
    if tr["status"] < 0:
        return dict(truth=tr, e=None)
    b = objective(*args, np.float64, jitter_rounds)
    cc = linalg(*args, jitter_rounds, points=None if pts is None else (*pts, zq))
    eb, ec = errors(b, tr), errors(cc, tr)
    if pts is not None:
        tr["post"] = posterior(*args, *pts, zq, np.longdouble, jitter_rounds)
        bp = posterior(*args, *pts, zq, np.float64, jitter_rounds)
        eb.update(post_errors(bp, tr["post"]))
        ec.update(post_errors(cc, tr["post"]))
    return dict(truth=tr, e={k: [eb[k], ec[k]] for k in eb})


def cap_of(output):
    return NLML_BUDGET_CAP if output == "nlml" else GRAD_BUDGET_CAP


def budgets(r):
    """{output: budget} of a programs_for / programs_of result (never clipped: test_warp_truth.py asserts every one is under its cap)"""
    return {k: budget(v, M_WARP) for k, v in r["e"].items()}


def programs_of(c, p, jitter_rounds=0):
    """programs_for on the case's seeded warp and points(c, p), computed once per process"""
    key = (c["id"], p, jitter_rounds)
    if key not in _PROGRAMS:
        _PROGRAMS[key] = programs_for(c, p, c["psi"][p], c["kind"], jitter_rounds, points(c, p), c["zq"])
    return _PROGRAMS[key]


def truth_of(c, p, jitter_rounds=0):
    return programs_of(c, p, jitter_rounds)["truth"]


def budget_of(c, p, jitter_rounds=0):
    """(truth dict, {output: budget}) of patient p of a case; truth status -1: budgets None"""
    r = programs_of(c, p, jitter_rounds)
    if r["e"] is None:
        return r["truth"], None
    return r["truth"], budgets(r)
