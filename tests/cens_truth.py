"""Extended-precision definition of the nlml, its gradient and the posterior with lab values reported at a detection limit (censored
observations), by expectation propagation (EP): what a device call for them is to be held to (there is none yet: DESIGN section
4.7t).  Built on nlml_truth.gram with nlml_truth's hand-written factor and triangular inverse,
basis_truth._chol_or_none (the pivot rule of A) and loo_grad_truth.grad_from_w, independent of oracle/.

Every observation row carries a code: 0 observed; BELOW (-1): the true noisy value is <= y, which holds the limit; ABOVE (+1): it is
>= y.  y = H beta + f + noise with H the indicator columns of the c censored rows (the caller's order) and beta_k = y_k - y*_k, the
distance of the true noisy value y*_k below the reported limit: the basis calls' model with the constraint s_k beta_k >= 0
(s_k = +1 BELOW, -1 ABOVE) in place of a Gaussian prior.  With K the matrix that is factored (all n rows, noise on every diagonal entry,
jitter rounds included), P = K^-1, z = L^-1 y, G = L^-1 H (column k: column row_k of L^-1), alpha_c = G^T z = (P y)_c:

    the Gaussian factor of beta has precision M = G^T G = P_cc and natural shift +alpha_c (exp(-(y - H beta)^T P (y - H beta) / 2) =
    exp(-beta^T M beta / 2 + beta^T alpha_c + const)); the sites are N(beta_k; nu~_k / tau~_k, 1 / tau~_k) up to scale, tau~_k >= 0
    posterior of beta   A = diag(tau~) + M,  h = nu~ + alpha_c,  beta ~ N(A^-1 h, A^-1)
    cavity of site k    tau_- = 1 / (A^-1)_kk - tau~_k,  nu_- = (A^-1 h)_k / (A^-1)_kk - nu~_k,  sigma_-^2 = 1 / tau_-,  mu_- = nu_- / tau_-
    site update         z = s_k mu_- / sigma_-,  r = phi(z) / Phi(z),  d = z + r,  g = r d,  v = 1 - g,  mu^ = mu_- + s_k sigma_- r,
                        sigma^^2 = sigma_-^2 v; moment matching in a form that does not cancel:  tau~_k = tau_- g / v,
                        nu~_k = tau_- s_k sigma_- (z g + r) / v, with z g + r = d - z v (tail5: how r, d, g, v are formed far below zero)
    sweeps              sites in ascending row order of the caller's observation order; after each site the rank-one update
                        A^-1 -= delta s s^T (s = column k of A^-1, delta = dtau / (1 + dtau (A^-1)_kk)) and A^-1 h += s (dnu - delta ((A^-1 h)_k
                        + dnu (A^-1)_kk)); at the end of every sweep A is factored again from the sites (R&W Alg. 3.5) and A^-1, A^-1 h
                        are rebuilt.  Cold start tau~ = nu~ = 0 (one rebuild before the first sweep).
    stopping            after a sweep: every site moved by |dtau| <= CENS_TOL (tau~ + M_kk) and |dnu| <= CENS_TOL (|nu~| + sqrt(M_kk))
                        (M_kk and sqrt(M_kk): the scales of a precision and of a natural shift of beta_k): the rule "device", what an fp64
                        program can meet.  MEDGP_CENS_MAX_SWEEPS sweeps without it: status -1.  rule "exact" (the truth): until no site moves by more than 2^-60 on those scales, or by less than
                        2^-54 and no longer by less than half of the sweep before (what rounding leaves of a strongly binding site).
    objective           nlml = quad / 2 + log|K| / 2 + log|A| / 2 + (n - c) log(2 PI) / 2
                               - sum_k [log Phi(z_k) + log(1 + tau~_k sigma_-k^2) / 2 + (tau~_k mu_-k - nu~_k)^2 / (2 tau~_k (1 + tau~_k sigma_-k^2))]
                        quad = |z - G beta^|^2 + sum_{tau~_k > 0} (tau~_k beta^_k - nu~_k)^2 / tau~_k   (the basis call's with lam = tau~,
                        b0 = nu~ / tau~); the last term of the bracket is 0 where tau~_k = 0; the cavities from the rebuilt A^-1
    gradient            alpha~ = P (y - H beta^),  W~ = P - P H A^-1 H^T P - alpha~ alpha~^T,  grad_h = tr(W~ dK/dtheta_h) / 2: the implicit
                        terms vanish at the fixed point (R&W 5.5.2, Seeger 2005)
    imputations         imp_mean_k = y_k - beta^_k,  imp_var_k = (A^-1)_kk: the EP posterior of the true noisy value of censored row k
    posterior at (m*, t*), V = L^-1 k*, r = -G^T V:  mean = V^T z + r^T beta^,  var = k** - V^T V + sigma^2 + r^T A^-1 r

status -1: n < min_n (3 for the objective, 1 for the posterior), a failed pivot of A, a cavity that is not positive or a site that is
not finite, or EP not converged.  More than CENS_MAX censored rows is the caller's error.

Tail functions in the working precision, no library: erfcx(x) = exp(x^2) erfc(x) for x >= 0 by the all-positive series of erf below 1
and by the continued fraction 1 / (sqrt(pi) (x + (1/2) / (x + 1 / (x + (3/2) / (x + ...))))) from 1 on; log Phi and phi / Phi from it
(test_cens_truth.py holds them to scipy.special.log_ndtr where scipy is importable).

The two legitimate fp64 programs of the budget, both with the rule "device": (b) this code in float64; (c) `linalg`: float64
through numpy.linalg on K (inv, slogdet), M = H^T P H, A^-1 rebuilt by inv every sweep, the quadratic form as y^T P y - h^T A^-1 h +
sum nu~^2 / tau~.  E is their distance from the long-double truth at the exact fixed point: it contains what the early stop leaves.

Error scales.  nlml: |nlml| floored at 1e-3 of its largest part.  grad: error_of's rule.  site: tau~_k on tau~_k + M_kk, nu~_k on
|nu~_k| + sqrt(M_kk) (the scales of the stopping rule).  imp_mean: |y_k| + |beta^_k|; imp_var: itself; each floored at 1e-3 of the
largest of its array.  Posterior mean and var: the sum of the absolute values of their terms per point.
"""
import numpy as np

import loo_grad_truth as LG
import nlml_truth as T
import posterior_jvp_truth as PJ
from basis_truth import _chol_or_none
from mean_truth import error_of, scale_of   # noqa: F401
from nlml_truth import GRAD_BUDGET_CAP, NLML_BUDGET_CAP, U64, budget, spread   # noqa: F401

BELOW, ABOVE = -1, 1                 # MEDGP_CENS_BELOW, MEDGP_CENS_ABOVE
CENS_MAX = 64                        # MEDGP_CENS_MAX: censored rows of a patient
MEDGP_CENS_MAX_SWEEPS = 64           # sweeps without convergence: status -1
CENS_TOL = 2.0 ** -42                # the stopping rule "device" (above)
EXACT_TOL = 2.0 ** -60               # the truth's
EXACT_STALL = 2.0 ** -54             # ... or, below this, until the movement stops shrinking (rounding of a strongly binding site)
EXACT_MAX_SWEEPS = 4 * MEDGP_CENS_MAX_SWEEPS

# ---- the budget (measured by tests/test_cens_truth.py::test_budget_factor_M_and_caps on the CPU programs only, never from device
# output).  M_CENS = the smallest power of two for which the two fp64 programs (b) and (c) stay within M / 4 times the smaller of
# their errors on every output of every patient of every case, zero and one jitter round (errors floored at U64).  The budget of an
# output of a patient is M_CENS * max(E_b, E_c, U64); the case set keeps every one under NLML_BUDGET_CAP (nlml) / GRAD_BUDGET_CAP
# (everything else) unclipped.  Provenance: DESIGN.md section 4.7t.
M_CENS = 128
MEASURED_SPREAD = 23.9
OBJ_OUTPUTS = ("nlml", "grad", "site", "imp_mean", "imp_var")
POST_OUTPUTS = ("mean", "var")

_PI_LD = "3.14159265358979323846264338327950288"


def _const(X):
    pi = X(_PI_LD) if X is np.longdouble else X(np.pi)
    return np.sqrt(pi), np.sqrt(X(2)), np.sqrt(2 * pi)


def _cf(x, X):
    """(f1, f2, f3) of the continued fraction erfcx(x) = 1 / (sqrt(pi) f1), f_k = x + (k / 2) / f_{k+1}, for x >= 1"""
    nterm = int(np.ceil(320.0 / float(x * x))) + 8      # the tail beyond it is below 2^-70 of the value
    f = [x, x, x]
    for k in range(nterm, 0, -1):
        f = [x + (X(k) / 2) / f[0], f[0], f[1]]
    return f


def erfcx_pos(x, X):
    """exp(x^2) erfc(x) of a scalar x >= 0 in precision X"""
    sqpi = _const(X)[0]
    x = X(x)
    if x < 1:
        # erf(x) = 2 / sqrt(pi) exp(-x^2) sum_n 2^n x^(2 n + 1) / (1 3 5 .. (2 n + 1)): positive terms
        term, s, n = x, x, 0
        while True:
            n += 1
            term = term * 2 * x * x / (2 * n + 1)
            s_new = s + term
            if s_new == s:
                break
            s = s_new
        return np.exp(x * x) - 2 / sqpi * s
    return 1 / (sqpi * _cf(x, X)[0])


def tail5(z, X):
    """(log Phi(z), r = phi(z) / Phi(z), d = z + r, g = r d, v = 1 - g) of a scalar z in precision X, each formed without cancellation:
    far below zero r ~ -z, d ~ 1 / |z| and v ~ 1 / z^2, and from r alone d would lose z^2 and v z^4 units of rounding; the continued
    fraction gives them directly (x = -z / sqrt(2), c1 = f1 - x, c2 = f2 - x): r = sqrt(2) f1, d = 1 / (sqrt(2) f2), g = f1 / f2,
    v = (c2 - c1) / f2"""
    sqpi, sq2, sq2pi = _const(X)
    z = X(z)
    if z <= 0:
        x = -z / sq2
        if x >= 1:
            f1, f2, f3 = _cf(x, X)
            return -np.log(2 * sqpi * f1) - x * x, sq2 * f1, 1 / (sq2 * f2), f1 / f2, (1 / f3 - 1 / (2 * f2)) / f2
        ex = erfcx_pos(x, X)
        r = (2 / sq2pi) / ex
        return np.log(ex / 2) - x * x, r, z + r, r * (z + r), 1 - r * (z + r)
    x = z / sq2
    q = erfcx_pos(x, X) * np.exp(-x * x) / 2                 # 1 - Phi(z) <= 1/2
    r = np.exp(-x * x) / sq2pi / (1 - q)
    return np.log1p(-q), r, z + r, r * (z + r), 1 - r * (z + r)


def tail(z, X):
    """(log Phi(z), phi(z) / Phi(z)) of a scalar z in precision X, accurate for z down to -30 and below"""
    return tail5(z, X)[:2]


def _moment_match(skk, mk, tk, nk, s, X):
    """the new (tau~, nu~) of one site from (A^-1)_kk, (A^-1 h)_k and the old site; None: the cavity is not positive or something is not
    finite.  tau~ = tau_- g / v, nu~ = tau_- s sigma_- w / v with w = mu_- g / (s sigma_-) + r = z g + r, taken as d - z v for z <= 0 and as
    r + z g above (both sums of positive terms)"""
    tcav = 1 / skk - tk
    ncav = mk / skk - nk
    if not tcav > 0:
        return None
    sd = 1 / np.sqrt(tcav)
    zz = s * (ncav / tcav) / sd
    _, r, d, g, v = tail5(zz, X)
    w = d - zz * v if zz <= 0 else r + zz * g
    tn = tcav * g / v
    nn = tcav * s * sd * w / v
    if not (np.isfinite(tn) and np.isfinite(nn) and tn >= 0):
        return None
    return tn, nn


def _rebuild_chol(Mm, tau, h, X):
    LA = _chol_or_none(np.diag(tau) + Mm) if Mm.shape[0] else np.zeros((0, 0), X)
    if LA is None:
        return None
    Ti = T._tri_inverse(LA) if Mm.shape[0] else np.zeros((0, 0), X)
    return Ti.T @ Ti, Ti.T @ (Ti @ h), Ti, np.sum(np.log(np.diagonal(LA))) if Mm.shape[0] else X(0)


def _rebuild_inv(Mm, tau, h, X):
    A = np.diag(tau) + Mm
    if not Mm.shape[0]:
        return np.zeros((0, 0), X), np.zeros(0, X), None, X(0)
    S = np.linalg.inv(A)
    S = (S + S.T) / 2
    return S, S @ h, None, np.linalg.slogdet(A)[1] / 2


def ep(Mm, alc, s, X, rule="device", rebuild=_rebuild_chol):
    """the EP fixed point of the c sites: dict(status, tau, nu, S = A^-1, mu = A^-1 h, Ti, logA = log|A| / 2, sweeps, dev_sweeps);
    dev_sweeps: the sweep at which the device's rule was first met (None: never)"""
    c = Mm.shape[0]
    tau, nu = np.zeros(c, X), np.zeros(c, X)
    dM = np.diagonal(Mm).copy()
    rb = rebuild(Mm, tau, nu + alc, X)
    if rb is None:
        return dict(status=-1)
    S, mu, Ti, logA = rb
    tol = X(CENS_TOL if rule == "device" else EXACT_TOL)
    cap = MEDGP_CENS_MAX_SWEEPS if rule == "device" else EXACT_MAX_SWEEPS
    sweeps, dev_sweeps, done, prev = 0, (0 if c == 0 else None), c == 0, None
    while not done:
        if sweeps == cap:
            return dict(status=-1, sweeps=sweeps, dev_sweeps=dev_sweeps)
        sweeps += 1
        S, mu = S.copy(), mu.copy()
        rel, dev_conv = X(0), True
        for k in range(c):
            mm = _moment_match(S[k, k], mu[k], tau[k], nu[k], s[k], X)
            if mm is None:
                return dict(status=-1, sweeps=sweeps, dev_sweeps=dev_sweeps)
            tn, nn = mm
            dt, dn = tn - tau[k], nn - nu[k]
            st, sn = tn + dM[k], abs(nn) + np.sqrt(dM[k])
            rel = max(rel, abs(dt) / st, abs(dn) / sn)
            dev_conv = dev_conv and abs(dt) <= X(CENS_TOL) * st and abs(dn) <= X(CENS_TOL) * sn
            dl = dt / (1 + dt * S[k, k])
            sv = S[:, k].copy()
            cm = dn - dl * (mu[k] + dn * sv[k])
            S = S - dl * np.outer(sv, sv)
            mu = mu + sv * cm
            tau[k], nu[k] = tn, nn
        if dev_conv and dev_sweeps is None:
            dev_sweeps = sweeps
        rb = rebuild(Mm, tau, nu + alc, X)
        if rb is None:
            return dict(status=-1, sweeps=sweeps, dev_sweeps=dev_sweeps)
        S, mu, Ti, logA = rb
        # (the truth also stops where the movement has sunk into the rounding of the working precision and no longer shrinks)
        done = rel <= tol or (rule == "exact" and prev is not None and rel <= X(EXACT_STALL) and rel >= prev / 2)
        prev = rel
    return dict(status=0, tau=tau, nu=nu, S=S, mu=mu, Ti=Ti, logA=logA, sweeps=sweeps, dev_sweeps=dev_sweeps)


def _site_terms(r, s, X):
    """(sum of the site normalisers' bracket, its largest part) from the rebuilt A^-1 and A^-1 h"""
    tot, big = X(0), X(0)
    for k in range(r["tau"].shape[0]):
        tk, nk = r["tau"][k], r["nu"][k]
        tcav = 1 / r["S"][k, k] - tk
        ncav = r["mu"][k] / r["S"][k, k] - nk
        sd2, mu = 1 / tcav, ncav / tcav
        lz, _ = tail(s[k] * mu / np.sqrt(sd2), X)
        one = 1 + tk * sd2
        q = (tk * mu - nk) ** 2 / (2 * tk * one) if tk > 0 else X(0)
        tot = tot + (lz + np.log(one) / 2 + q)
        big = max(big, abs(lz), abs(np.log(one) / 2), abs(q))
    return tot, big


def codes(code, n):
    code = np.zeros(n, np.int64) if code is None else np.asarray(code, np.int64).reshape(n)
    assert np.all((code >= -1) & (code <= 1))
    idx = np.where(code != 0)[0]
    assert idx.shape[0] <= CENS_MAX
    return idx, -code[idx]          # s = +1 BELOW, -1 ABOVE


def objective(kidx, Q, D, R, meta, t, y, theta, code, dtype=np.longdouble, jitter_rounds=0, want_grad=True, min_n=3, want_parts=False,
              rule=None):
    """dict(status, nlml, nlml_mag, grad, site [c, 2] = (nu~, tau~), site_mag, imp_mean, imp_mean_mag, imp_var, sweeps, dev_sweeps
    [, parts]) in precision dtype; rule: "exact" for long double, "device" otherwise"""
    X = dtype
    rule = rule or ("exact" if X is np.longdouble else "device")
    t32 = np.asarray(t, np.float32)
    n = t32.shape[0]
    if n < min_n:
        return dict(status=-1)
    idx, s = codes(code, n)
    c = idx.shape[0]
    yy = np.asarray(y, np.float32).astype(X)
    K = T.gram(kidx, Q, D, R, meta, t32, theta, X, jitter_rounds)
    L = T._chol_columns(K)
    Li = T._tri_inverse(L)
    z = Li @ yy
    G = Li[:, idx]
    Mm = G.T @ G
    alc = G.T @ z
    r = ep(Mm, alc, s.astype(X), X, rule)
    if r["status"] < 0:
        return dict(status=-1, sweeps=r.get("sweeps"), dev_sweeps=r.get("dev_sweeps"))
    beta, tau, nu = r["mu"], r["tau"], r["nu"]
    res = z - G @ beta
    pos = tau > 0
    pen = np.sum((tau[pos] * beta[pos] - nu[pos]) ** 2 / tau[pos])
    quad = res @ res + pen
    logK = np.sum(np.log(np.diagonal(L)))
    log2pi = np.log(2 * X(np.float64(T.REF_PI)))
    sites, sbig = _site_terms(r, s.astype(X), X)
    nlml = quad / 2 + logK + r["logA"] + (n - c) * log2pi / 2 - sites
    parts = [quad / 2, logK, r["logA"], (n - c) * log2pi / 2, sbig]
    dM = np.diagonal(Mm)
    out = dict(status=jitter_rounds, nlml=nlml, nlml_mag=max(abs(nlml), X(1e-3) * max(abs(p) for p in parts)), grad=None,
               site=np.stack([nu, tau], axis=1), site_mag=np.stack([np.abs(nu) + np.sqrt(dM), tau + dM], axis=1),
               imp_mean=yy[idx] - beta, imp_mean_mag=np.abs(yy[idx]) + np.abs(beta), imp_var=np.diagonal(r["S"]).copy(),
               sweeps=r["sweeps"], dev_sweeps=r["dev_sweeps"])
    if want_grad or want_parts:
        PH = Li.T @ G
        at = Li.T @ res
        Pm = PH @ r["Ti"].T
        W = T._gram_upper_product(Li) - Pm @ Pm.T - np.outer(at, at)
        if want_grad:
            out["grad"] = LG.grad_from_w(kidx, Q, D, R, meta, t32, theta, W, X, "blocks")
        if want_parts:
            out["parts"] = dict(Li=Li, z=z, G=G, Ti=r["Ti"], S=r["S"], beta=beta, W=W, alpha_t=at, idx=idx, s=s, M=Mm, alc=alc)
    return out


def posterior(kidx, Q, D, R, meta, t, y, theta, code, meta2, t2, dtype=np.longdouble, jitter_rounds=0):
    """dict(status, mean, var, mag_mean, mag_var, sweeps)"""
    X = dtype
    r = objective(kidx, Q, D, R, meta, t, y, theta, code, X, jitter_rounds, want_grad=False, min_n=1, want_parts=True)
    if r["status"] < 0:
        return r
    q = r["parts"]
    Ks, kss, s2 = PJ.cross_gram(kidx, Q, D, R, meta, np.asarray(t, np.float32), theta, meta2, t2, X)
    V = q["Li"] @ Ks
    rr = -(V.T @ q["G"])
    u = rr @ q["Ti"].T
    extra = np.sum(u * u, axis=1)
    vv = np.sum(V * V, axis=0)
    return dict(status=r["status"], mean=V.T @ q["z"] + rr @ q["beta"], var=kss - vv + s2 + extra,
                mag_mean=np.abs(V).T @ np.abs(q["z"]) + (np.abs(V).T @ np.abs(q["G"])) @ np.abs(q["beta"]), mag_var=np.abs(kss) + vv + s2 + extra,
                sweeps=r["sweeps"])


def linalg(kidx, Q, D, R, meta, t, y, theta, code, jitter_rounds=0, points=None):
    """program (c): float64 through numpy.linalg on K, A^-1 by inv every sweep, the device's stopping rule.  points = (meta2, t2):
    also mean, var"""
    X = np.float64
    t32 = np.asarray(t, np.float32)
    n = t32.shape[0]
    idx, s = codes(code, n)
    c = idx.shape[0]
    yy = np.asarray(y, np.float32).astype(X)
    K = T.gram(kidx, Q, D, R, meta, t32, theta, X, jitter_rounds)
    P = np.linalg.inv(K)
    P = (P + P.T) / 2
    al = P @ yy
    Mm = P[np.ix_(idx, idx)]
    r = ep(Mm, al[idx], s.astype(X), X, "device", _rebuild_inv)
    if r["status"] < 0:
        return dict(status=-1)
    beta, tau, nu = r["mu"], r["tau"], r["nu"]
    h = nu + al[idx]
    pos = tau > 0
    quad = yy @ al - h @ beta + np.sum(nu[pos] ** 2 / tau[pos])
    sites, _ = _site_terms(r, s.astype(X), X)
    nlml = quad / 2 + np.linalg.slogdet(K)[1] / 2 + r["logA"] + (n - c) * np.log(2 * T.REF_PI) / 2 - sites
    PH = P[:, idx]
    at = al - PH @ beta
    W = P - PH @ r["S"] @ PH.T - np.outer(at, at)
    out = dict(status=jitter_rounds, nlml=nlml, grad=LG.grad_from_w(kidx, Q, D, R, meta, t32, theta, W, X, "blocks"),
               site=np.stack([nu, tau], axis=1), imp_mean=yy[idx] - beta, imp_var=np.diagonal(r["S"]).copy(), sweeps=r["sweeps"])
    if points is not None:
        Ks, kss, s2 = PJ.cross_gram(kidx, Q, D, R, meta, t32, theta, points[0], points[1], X)
        rr = -(Ks.T @ PH)
        out["mean"] = Ks.T @ al + rr @ beta
        out["var"] = kss - np.sum(Ks * (P @ Ks), axis=0) + s2 + np.sum((rr @ r["S"]) * rr, axis=1)
    return out


# ---- errors ------------------------------------------------------------------------------------------------------------------------

def errors(got, truth):
    """{output: E} of a result dict against the truth dict of `objective` (outputs the result does not carry are left out); the
    arrays of got may be padded beyond c"""
    e = {}
    c = truth["site"].shape[0]
    for k in OBJ_OUTPUTS:
        if got.get(k) is None or truth.get(k) is None:
            continue
        g = got[k] if k in ("nlml", "grad") else np.asarray(got[k])[:c]
        mag = {"nlml": truth["nlml_mag"], "site": truth["site_mag"], "imp_mean": truth["imp_mean_mag"]}.get(k)
        e[k] = error_of(g, truth[k], mag)
    return e


def post_errors(got, post):
    return {k: error_of(got[k], post[k], post["mag_" + k]) for k in POST_OUTPUTS if got.get(k) is not None}


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# (id, kidx, Q, D, R, [(n, random_patient mode, placement)]): the smallest shapes at which the new kernels can go wrong -- n = 3 (the
# n > 2 guard's edge), 17, 63 / 64 / 65 (the 64-row block edge of the library's panels), 130, 200; D = 1 through SE and SM, 3, 24; every case
# carries c = 0, 1, 7 and 64 in one batch.  "shuffled" patients arrive with the covariates interleaved: the grouped row of a censored
# row is not its caller's row.  Placements (rows are GROUPED rows, mapped back to the caller's order; where not said, a BELOW limit
# lies U(0.2, 1.5) above the drawn value, an ABOVE limit as far below):
#   none      c = 0
#   one       c = 1: the last grouped row, BELOW
#   edges7    c = 7: the first and the last grouped row, rows 62, 63, 64 where n has them (else the rows before the last), two more drawn
#   far7      c = 7 as edges7, BELOW; the limit of the sixth 8 noise standard deviations ABOVE where the GP puts the value given the others
#             (a site that stays at ~0), that of the seventh 8 BELOW it (a strongly binding one)
#   cov       every row of the covariate with the fewest (>= 1) rows, BELOW and ABOVE alternating (at most 64 rows)
#   same7     c = 7 with two censored rows brought to one time stamp (same covariate, adjacent grouped rows), signs mixed
#   full64    c = 64: rows 63, 64, 65, the first, the last and 59 drawn, signs mixed
_SPECS = [
    ("se", 0, 1, 1, 0, [(3, "plain", "one"), (17, "plain", "none"), (64, "plain", "edges7"), (130, "plain", "full64")]),
    ("sm_Q3", 8, 3, 1, 0, [(17, "plain", "one"), (65, "plain", "far7"), (200, "plain", "full64"), (63, "plain", "none"), (130, "plain", "same7")]),
    ("lmc_D3_Q5", 7, 5, 3, 2, [(3, "plain", "one"), (63, "shuffled", "edges7"), (64, "shuffled", "none"), (65, "plain", "cov"),
                              (130, "shuffled", "full64"), (200, "shuffled", "same7")]),
    ("lmc_D24", 7, 5, 24, 8, [(130, "missing", "one"), (64, "shuffled", "far7"), (200, "shuffled", "full64"), (65, "plain", "none"),
                             (130, "shuffled", "cov")]),
]
CASE_IDS = [s[0] for s in _SPECS]
JITTER_CASE, JITTER_PS = "lmc_D3_Q5", [1, 3, 4, 5]      # the patients the budget also measures with one jitter round
# hyper draw of a patient where it is not the first (nlml_truth.DRAWS's rule: a draw whose budget from the CPU programs alone would
# exceed a cap, or on which the two programs are more than M_CENS / 4 apart, is replaced by the next one, on the CPU)
DRAWS = {}
_CASES = {}


def _meta(kidx, meta, n):
    return np.asarray(meta, np.int64) if kidx == 7 else np.zeros(n, np.int64)


def grouping(kidx, meta, n):
    """perm[i] = the caller's row of grouped row i (stable by covariate, as the library groups)"""
    return np.argsort(_meta(kidx, meta, n), kind="stable")


def _place(g, kidx, Q, D, R, m, t, y, theta, kind):
    """(t, y, code) of a patient under a placement: y holds the limits at the censored rows"""
    n = t.shape[0]
    perm = grouping(kidx, m, n)
    mm = _meta(kidx, m, n)
    code = np.zeros(n, np.int8)
    t, y = t.copy(), y.copy()
    if kind == "none":
        return t, y, code

    def shift(rows, signs):
        for i, sg in zip(rows, signs):
            code[i] = sg
            y[i] = np.float32(y[i] - sg * g.uniform(0.2, 1.5))     # BELOW (-1): the limit above the drawn value
    pick = lambda k, avoid: list(g.choice([i for i in range(n) if i not in avoid], size=k, replace=False))   # noqa: E731
    if kind == "one":
        shift([perm[n - 1]], [BELOW])
    elif kind in ("edges7", "far7", "same7"):
        gr = [0, n - 1] + ([62, 63, 64] if n > 65 else [n - 4, n - 3, n - 2])
        gr += pick(2, gr)
        rows = [perm[i] for i in gr]
        if kind == "same7":
            a, b = sorted(gr)[2], sorted(gr)[3]               # adjacent grouped rows 62, 63 (or n - 4, n - 3)
            if mm[perm[a]] == mm[perm[b]]:
                t[perm[b]] = t[perm[a]]
        signs = [BELOW] * 7 if kind == "far7" else [BELOW if j % 2 == 0 else ABOVE for j in range(7)]
        shift(rows, signs)
        if kind == "far7":
            K = T.gram(kidx, Q, D, R, m, t, theta, np.float64)
            P = np.linalg.inv(K)
            yd = np.asarray(y, np.float64)
            for j, far in ((5, +8.0), (6, -8.0)):                # the two drawn rows
                i = rows[j]
                loo = yd[i] - (P @ yd)[i] / P[i, i]            # where the GP puts row i given the others
                y[i] = np.float32(loo + far * np.sqrt(noise_var(kidx, Q, D, R, theta, mm[i])))
    elif kind == "cov":
        cnt = np.bincount(mm, minlength=D)
        d = int(np.argmin(np.where(cnt > 0, cnt, n + 1)))
        rows = [i for i in range(n) if mm[i] == d][:CENS_MAX]
        shift(rows, [BELOW if j % 2 == 0 else ABOVE for j in range(len(rows))])
    elif kind == "full64":
        gr = [0, n - 1, 63, 64, 65]
        gr += pick(59, gr)
        shift([perm[i] for i in gr], [BELOW if j % 3 else ABOVE for j in range(64)])
    else:
        raise ValueError(kind)
    return t, y, code


def noise_var(kidx, Q, D, R, theta, d):
    """the noise variance of covariate d: what the Gram matrix carries on the diagonal beyond the kernel, read off it"""
    m1 = np.full(2, d, np.int32) if kidx == 7 else None
    K2 = T.gram(kidx, Q, D, R, m1, np.zeros(2, np.float32), theta, np.float64)     # two rows at one time stamp
    return float(K2[0, 0] - K2[0, 1])


def case(cid):
    """dict(id, kidx, Q, D, R, pts, th, code, kind) from seeds alone"""
    if cid not in _CASES:
        from medgp_amd import synth
        from random_patients import random_patient
        ci = CASE_IDS.index(cid)
        _, kidx, Q, D, R, spec = _SPECS[ci]
        g = T._philox(20262001, ci)
        pts, th, cds, kinds = [], [], [], []
        for p, (n, mode, kind) in enumerate(spec):
            if kidx == 7:
                m, t, _ = random_patient(g, D, n, mode)
            else:
                m, t = None, np.sort(g.uniform(0.0, 200.0, size=n)).astype(np.float32)
            theta = synth.theta(5016 + 1000 * DRAWS.get((cid, p), 0), 100 * ci + p, kidx, Q, D, R)
            K = T.gram(kidx, Q, D, R, m, t, theta, np.float64)
            y = (np.linalg.cholesky(K) @ g.standard_normal(n)).astype(np.float32)      # a sample of the model: well specified
            t, y, code = _place(g, kidx, Q, D, R, m, t, y, theta, kind)
            pts.append((m, t, y))
            th.append(theta)
            cds.append(code)
            kinds.append(kind)
        _CASES[cid] = dict(id=cid, kidx=kidx, Q=Q, D=D, R=R, pts=pts, th=th, code=cds, kind=kinds)
    return _CASES[cid]


def fam(c):
    return c["kidx"], c["Q"], c["D"], c["R"]


def patients():
    return [(cid, p) for cid in CASE_IDS for p in range(len(case(cid)["pts"]))]


def points(c, p, count=24):
    """(meta2 or None, t2) of patient p from seeds alone: times from 24 h before the first to 24 h after the last observation,
    covariates uniform over all D; the first four points AT the time stamps (and covariates) of censored rows where there are any"""
    ci = CASE_IDS.index(c["id"])
    g = T._philox(20262002, 1000 * ci + p)
    m, t, _ = c["pts"][p]
    t2 = g.uniform(float(t.min()) - 24.0, float(t.max()) + 24.0, size=count).astype(np.float32)
    m2 = g.integers(0, c["D"], size=count).astype(np.int32) if c["kidx"] == 7 else None
    idx = np.where(c["code"][p] != 0)[0][:4]
    for j, i in enumerate(idx):
        t2[j] = t[i]
        if m2 is not None:
            m2[j] = m[i]
    return m2, t2


_PROGRAMS = {}


def programs_for(c, p, code, jitter_rounds=0, pts=None):
    """dict(truth, b, e = {output: [E_b, E_c]}) of the two fp64 programs on patient p of a case under the table `code`; pts =
    (meta2, t2): also the posterior's mean, var (truth["post"]).  Not cached."""
    m, t, y = c["pts"][p]
    args = (*fam(c), m, t, y, c["th"][p], code)
    tr = objective(*args, np.longdouble, jitter_rounds)
    if tr["status"] < 0:
        return dict(truth=tr, b=None, e=None)
    b = objective(*args, np.float64, jitter_rounds)
    cc = linalg(*args, jitter_rounds, points=pts)
    assert b["status"] >= 0 and cc["status"] >= 0
    eb, ec = errors(b, tr), errors(cc, tr)
    if pts is not None:
        tr["post"] = posterior(*args, *pts, np.longdouble, jitter_rounds)
        bp = posterior(*args, *pts, np.float64, jitter_rounds)
        eb.update(post_errors(bp, tr["post"]))
        ec.update(post_errors(cc, tr["post"]))
    return dict(truth=tr, b=b, c=cc, e={k: [eb[k], ec[k]] for k in eb})


def cap_of(output):
    return NLML_BUDGET_CAP if output == "nlml" else GRAD_BUDGET_CAP


def budgets(r):
    """{output: budget} of a programs_for / programs_of result (never clipped: test_cens_truth.py asserts every one is under its cap)"""
    return {k: budget(v, M_CENS) for k, v in r["e"].items()}


def programs_of(c, p, jitter_rounds=0):
    """programs_for on the case's seeded table and points(c, p), computed once per process"""
    key = (c["id"], p, jitter_rounds)
    if key not in _PROGRAMS:
        _PROGRAMS[key] = programs_for(c, p, c["code"][p], jitter_rounds, points(c, p))
    return _PROGRAMS[key]


def truth_of(c, p, jitter_rounds=0):
    return programs_of(c, p, jitter_rounds)["truth"]


def budget_of(c, p, jitter_rounds=0):
    """(truth dict, {output: budget}) of patient p of a case; truth status -1: budgets None"""
    r = programs_of(c, p, jitter_rounds)
    if r["e"] is None:
        return r["truth"], None
    return r["truth"], budgets(r)
