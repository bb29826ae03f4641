"""Lab values reported at a detection limit -- troponin "< 0.01", CRP "< 3", lactate "> 20".  A row coded BELOW (-1) says that the
true noisy value is at or below the reported y, which holds the limit; ABOVE (+1) that it is at or above; 0 is an ordinary observation.
Every call of the library treats such a row as an exact observation AT the limit; the correct model only states that the value lies
beyond it, and expectation propagation (EP) replaces each such statement by a Gaussian site (nu~, tau~).  The definition, in long double
and with its error budget, is tests/cens_truth.py; this module is its numpy side, for dense covariance matrices of
small n.  There is NO device call for it yet (DESIGN section 4.7t says why): nothing here touches the GPU.

    from_limits       reported values and per-covariate detection limits -> (y, code): the values clipped to the limits
    codes_from_flags  "<" / ">" flags of a lab feed -> code
    ep_dense          EP on a dense covariance matrix: sites, the posterior of limit minus value, the imputations (imp_mean, imp_var)
    impute            imp_mean / imp_var / site -> the truncated normal of every censored row (its location and scale, its mean and
                      variance, quantiles), in the caller's units
    exact_single      the closed form for ONE censored row, -log N(y_o; 0, K_oo) - log Phi(.): EP is exact there
    naive_bias        how far the posterior moves, and how much narrower it gets, when the limits are treated as observations
"""
import math

import numpy as np

BELOW, ABOVE = -1, 1          # MEDGP_CENS_BELOW, MEDGP_CENS_ABOVE
CENS_MAX = 64                 # censored rows of a patient (tests/cens_truth.py: CENS_MAX)
MAX_SWEEPS = 64               # sweeps without convergence: an error (MEDGP_CENS_MAX_SWEEPS)
TOL = 2.0 ** -42              # the stopping rule (tests/cens_truth.py: CENS_TOL)


def from_limits(y, lower=None, upper=None, meta=None):
    """(y, code): the reported values clipped to the detection limits and the code of every row.  lower / upper: a scalar or one limit
    per covariate ([D], indexed by meta; NaN or None: the covariate has no such limit), in the units of y.  A value at or below its
    lower limit becomes the limit with code BELOW ("< limit"), at or above its upper limit the limit with code ABOVE."""
    y = np.array(y, dtype=np.float64)
    n = y.shape[0]
    m = np.zeros(n, np.int64) if meta is None else np.asarray(meta, np.int64)
    code = np.zeros(n, np.int8)
    for lim, cd in ((lower, BELOW), (upper, ABOVE)):
        if lim is None:
            continue
        la = np.asarray(lim, np.float64)
        li = np.full(n, float(la)) if la.ndim == 0 else la[m]
        hit = (y <= li) if cd == BELOW else (y >= li)
        hit &= ~np.isnan(li)
        if np.any(hit & (code != 0)):
            raise ValueError("a value lies beyond both of its limits: lower >= upper")
        y[hit] = li[hit]
        code[hit] = cd
    return y, code


def codes_from_flags(flags):
    """int8 codes from the comparison flags of a lab feed: "<" or "<=" -> BELOW, ">" or ">=" -> ABOVE, "", "=", None -> 0"""
    table = {"<": BELOW, "<=": BELOW, ">": ABOVE, ">=": ABOVE, "": 0, "=": 0, None: 0}
    out = np.zeros(len(flags), np.int8)
    for i, f in enumerate(flags):
        key = f.strip() if isinstance(f, str) else f
        if key not in table:
            raise ValueError(f"flag {f!r} at row {i} is none of '<', '<=', '>', '>=', '=', ''")
        out[i] = table[key]
    return out


# ---- the tail of the normal distribution, accurate far below zero ---------------------------------------------------------------

def _cf(x):
    """(f1, f2, f3) of the continued fraction erfcx(x) = 1 / (sqrt(pi) f1), f_k = x + (k / 2) / f_{k+1}, x >= 1"""
    f = [x, x, x]
    for k in range(int(math.ceil(320.0 / (x * x))) + 8, 0, -1):
        f = [x + 0.5 * k / f[0], f[0], f[1]]
    return f


def _erfcx_pos(x):
    """exp(x^2) erfc(x), x >= 0: the positive series of erf below 1, the continued fraction from 1 on"""
    if x < 1.0:
        term = s = x
        n = 0
        while True:
            n += 1
            term *= 2.0 * x * x / (2 * n + 1)
            if s + term == s:
                break
            s += term
        return math.exp(x * x) - 2.0 / math.sqrt(math.pi) * s
    return 1.0 / (math.sqrt(math.pi) * _cf(x)[0])


def tail5(z):
    """(log Phi(z), r = phi(z) / Phi(z), d = z + r, g = r d, v = 1 - g) of a scalar, without underflow or cancellation for z far below
    zero (there r ~ -z, d ~ 1 / |z|, v ~ 1 / z^2 come from the continued fraction directly: tests/cens_truth.py: tail5)"""
    z = float(z)
    if z <= 0.0:
        x = -z / math.sqrt(2.0)
        if x >= 1.0:
            f1, f2, f3 = _cf(x)
            return -math.log(2.0 * math.sqrt(math.pi) * f1) - x * x, math.sqrt(2.0) * f1, 1.0 / (math.sqrt(2.0) * f2), f1 / f2, (1.0 / f3 - 0.5 / f2) / f2
        ex = _erfcx_pos(x)
        lz, r = math.log(ex / 2.0) - x * x, math.sqrt(2.0 / math.pi) / ex
    else:
        x = z / math.sqrt(2.0)
        q = _erfcx_pos(x) * math.exp(-x * x) / 2.0
        lz, r = math.log1p(-q), math.exp(-x * x) / math.sqrt(2.0 * math.pi) / (1.0 - q)
    return lz, r, z + r, r * (z + r), 1.0 - r * (z + r)


def log_cdf_and_ratio(z):
    """(log Phi(z), phi(z) / Phi(z)) of a scalar, without underflow for z far below zero"""
    return tail5(z)[:2]


def _norm_ppf(p):
    z = 0.0
    for _ in range(80):   # Newton steps on erf
        z -= (0.5 * math.erfc(-z / math.sqrt(2.0)) - p) / max(math.exp(-z * z / 2) / math.sqrt(2 * math.pi), 1e-300)
    return z


def impute(limit, code, imp_mean, imp_var, site, center=0.0, scale=1.0, probs=None):
    """The distribution of the true value of every censored row of ONE patient.  limit: the uploaded y at the censored rows [c] (the
    caller's order); code [c] (BELOW / ABOVE); imp_mean, imp_var [>= c], site [>= c, 2]: as ep_dense returns them.  EP's tilted distribution of a censored row is a normal N(loc, sd^2) -- the cavity: what all OTHER
    rows say about this one -- truncated at the limit; imp_mean and imp_var are its mean and variance.  Returns dict(loc, sd, mean,
    var [, quant [c, len(probs)]]) in the caller's units: value = center + scale * (model value), center / scale scalars or [c]."""
    limit, code = np.asarray(limit, np.float64), np.asarray(code, np.int64)
    c = limit.shape[0]
    im, iv, st = np.asarray(imp_mean, np.float64)[:c], np.asarray(imp_var, np.float64)[:c], np.asarray(site, np.float64)[:c]
    if np.any(code == 0):
        raise ValueError("impute takes the censored rows only")
    s = -code.astype(np.float64)                       # +1 BELOW: beta = limit - value >= 0
    tcav = 1.0 / iv - st[:, 1]
    ncav = (limit - im) / iv - st[:, 0]                # the cavity of beta
    sd = 1.0 / np.sqrt(tcav)
    mu = ncav / tcav
    loc = limit - mu                                   # the cavity of the value
    mean, var = np.empty(c), np.empty(c)
    for k in range(c):
        z = s[k] * mu[k] / sd[k]
        _, r, _, _, v = tail5(z)
        mean[k] = limit[k] - (mu[k] + s[k] * sd[k] * r)
        var[k] = sd[k] ** 2 * v
    center, scale = np.asarray(center, np.float64), np.asarray(scale, np.float64)
    out = dict(loc=center + scale * loc, sd=scale * sd, mean=center + scale * mean, var=scale ** 2 * var)
    if probs is not None:
        q = np.empty((c, len(probs)))
        for k in range(c):
            # BELOW: value <= limit, CDF F(v) = Phi((v - loc) / sd) / Phi((limit - loc) / sd); ABOVE: by reflection
            a = s[k] * (limit[k] - loc[k]) / sd[k]
            pa = 0.5 * math.erfc(-a / math.sqrt(2.0))
            for j, p in enumerate(probs):
                pp = p if s[k] > 0 else 1.0 - p
                q[k, j] = loc[k] + s[k] * sd[k] * _norm_ppf(pp * pa)
        out["quant"] = center.reshape(-1, 1) + scale.reshape(-1, 1) * q
    return out


def exact_single(K, y, code):
    """-log p of a patient with ONE censored row under a zero-mean normal with covariance K (noise on its diagonal):
    -log N(y_o; 0, K_oo) - log Phi(s (limit - m) / sd) with (m, sd^2) the conditional of the censored row given the observed ones."""
    K, y, code = np.asarray(K, np.float64), np.asarray(y, np.float64), np.asarray(code, np.int64)
    k = np.where(code != 0)[0]
    if k.shape[0] != 1:
        raise ValueError("exact_single takes exactly one censored row")
    k = int(k[0])
    o = np.arange(y.shape[0]) != k
    Koo = K[np.ix_(o, o)]
    L = np.linalg.cholesky(Koo)
    w = np.linalg.solve(L, y[o])
    v = np.linalg.solve(L, K[o, k])
    m, var = v @ w, K[k, k] - v @ v
    lz, _ = log_cdf_and_ratio(-code[k] * (y[k] - m) / math.sqrt(var))
    return 0.5 * (w @ w) + np.sum(np.log(np.diag(L))) + 0.5 * int(o.sum()) * math.log(2 * math.pi) - lz


def ep_dense(K, y, code, max_sweeps=MAX_SWEEPS, tol=TOL):
    """EP by the definition's sweeps and stopping rule on a dense covariance matrix K (noise on its diagonal; small n).  Returns dict(site [c, 2] = (nu~, tau~), beta
    [c] = E(limit - value), cov [c, c], imp_mean, imp_var, sweeps, idx, P = K^-1, alpha = K^-1 y); raises ArithmeticError without
    convergence."""
    K, y, code = np.asarray(K, np.float64), np.asarray(y, np.float64), np.asarray(code, np.int64)
    idx = np.where(code != 0)[0]
    c = idx.shape[0]
    if c > CENS_MAX:
        raise ValueError(f"{c} censored rows, at most {CENS_MAX}")
    s = -code[idx].astype(np.float64)
    P = np.linalg.inv(K)
    P = (P + P.T) / 2
    al = P @ y
    M, alc = P[np.ix_(idx, idx)], al[idx]
    tau, nu = np.zeros(c), np.zeros(c)
    S = np.linalg.inv(M) if c else np.zeros((0, 0))
    mu = S @ alc
    sweeps, done = 0, c == 0
    while not done:
        if sweeps == max_sweeps:
            raise ArithmeticError("EP did not converge")
        sweeps += 1
        done = True
        for k in range(c):
            tcav, ncav = 1.0 / S[k, k] - tau[k], mu[k] / S[k, k] - nu[k]
            if not tcav > 0:
                raise ArithmeticError("a cavity is not positive")
            sd, m = 1.0 / math.sqrt(tcav), ncav / tcav
            z = s[k] * m / sd
            _, r, d, g, v = tail5(z)
            tn, nn = tcav * g / v, tcav * s[k] * sd * (d - z * v if z <= 0 else r + z * g) / v
            dt, dn = tn - tau[k], nn - nu[k]
            done = done and abs(dt) <= tol * (tn + M[k, k]) and abs(dn) <= tol * (abs(nn) + math.sqrt(M[k, k]))
            dl = dt / (1.0 + dt * S[k, k])
            sv = S[:, k].copy()
            cm = dn - dl * (mu[k] + dn * sv[k])
            S -= dl * np.outer(sv, sv)
            mu += sv * cm
            tau[k], nu[k] = tn, nn
        S = np.linalg.inv(np.diag(tau) + M)
        S = (S + S.T) / 2
        mu = S @ (nu + alc)
    return dict(site=np.stack([nu, tau], axis=1), beta=mu, cov=S, imp_mean=y[idx] - mu, imp_var=np.diag(S).copy(), sweeps=sweeps, idx=idx,
                P=P, alpha=al)


def naive_bias(K, y, code, Ks, kss):
    """What treating the limits as observations does to the posterior at test points.  K [n, n]: the covariance of the observations
    (noise on the diagonal); Ks [n, m]: their covariance with the points; kss [m]: the points' prior variance (with noise, if the
    prediction is of a noisy value).  Returns dict(mean_naive, var_naive, mean_cens, var_cens, shift = (mean_naive - mean_cens) /
    sqrt(var_cens), var_ratio = var_naive / var_cens): the naive posterior is pulled onto the limits (shift) and too narrow
    (var_ratio < 1).  A diagnostic on dense matrices, numpy only."""
    Ks, kss = np.asarray(Ks, np.float64), np.asarray(kss, np.float64)
    r = ep_dense(K, y, code)
    P, al, idx = r["P"], r["alpha"], r["idx"]
    mean_naive = Ks.T @ al
    var_naive = kss - np.sum(Ks * (P @ Ks), axis=0)
    rr = -(Ks.T @ P[:, idx])                           # r_j = -H^T P k*_j
    mean_cens = mean_naive + rr @ r["beta"]
    var_cens = var_naive + np.sum((rr @ r["cov"]) * rr, axis=1)
    return dict(mean_naive=mean_naive, var_naive=var_naive, mean_cens=mean_cens, var_cens=var_cens,
                shift=(mean_naive - mean_cens) / np.sqrt(var_cens), var_ratio=var_naive / var_cens)
