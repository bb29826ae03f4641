"""Per-observation noise scales and Student-t robust training: the numpy side of medgp_set_noise_scale, medgp_hetero_nlml_grad,
medgp_hetero_posterior_batch and medgp_robust_nlml_grad (include/medgp_hip.h; the definition is tests/hetero_truth.py).

Every other call gives all observations of covariate d the noise variance sigma^2_d.  A scale s_i > 0 per row makes it sigma^2_d s_i:

    from_replicates(counts)     an hourly value that is the mean of k monitor readings: s = 1 / k
    from_sd(sd, sigma)          a value whose own standard deviation is known (a second device, a point-of-care analyser): s = (sd / sigma)^2
    flagged(mask, factor)       values flagged as doubtful ("hemolysed"): s = factor where flagged, 1 elsewhere

and Context.set_noise_scale makes them resident for hetero_nlml_grad / hetero_posterior.  Where single values are grossly wrong without
a flag (a transcription error, a line flush, a motion artefact) the scales are LEARNED: Student-t noise written as a Gaussian scale
mixture, eps_i | tau_i ~ N(0, sigma^2_d / tau_i), tau_i ~ Gamma(nu_d / 2, nu_d / 2), with q(tau_i) = Gamma(a_d, a_d s_i),
a_d = (nu_d + 1) / 2.  Context.robust_nlml_grad makes `sweeps` E-steps s_i <- (nu_d + e_i) / (nu_d + 1), e_i = (resid_i^2 + fvar_i) /
sigma^2_d, and returns the negative evidence bound J(theta, nu, s) >= the exact Student-t nlml with its gradient in theta at the
scales it ends with (the VB-EM M-step gradient, no implicit terms dropped).  nu is not learned by gradient: select_nu scans a grid in
one call.

    fit(ctx, slots, theta0, nu, sweeps)    optimiser closures over theta that warm-start the scales from the previous evaluation
    select_nu(ctx, slot, theta, grid)      J over a grid of nu for one patient, one call
    outlier_weight(scale)                  1 / s: the weight of a row's precision in the posterior mean (near 0: the row was set aside)
    predictive_interval(...)               latent Gaussian plus Student-t noise, by quadrature
    dense(K, y, sigma2, nu, sweeps)        a float64 restatement for users without a device

numpy only.
"""
import math

import numpy as np

SCALE_MIN, SCALE_MAX = 2.0 ** -40, 2.0 ** 40     # the range medgp_set_noise_scale accepts


def _checked(s):
    s = np.asarray(s, dtype=np.float64)
    if not np.all(np.isfinite(s) & (s >= SCALE_MIN) & (s <= SCALE_MAX)):
        raise ValueError("a noise scale must be finite and lie in [2^-40, 2^40]")
    return s


def from_replicates(counts):
    """s = 1 / k for a value that is the mean of k readings"""
    k = np.asarray(counts, dtype=np.float64)
    if not np.all(k >= 1):
        raise ValueError("replicate counts are at least 1")
    return _checked(1.0 / k)


def from_sd(sd, sigma):
    """s = (sd / sigma)^2: sd the known standard deviation of each value, sigma the covariate's noise sd the model carries (a scalar, or
    one per row)"""
    return _checked((np.asarray(sd, dtype=np.float64) / np.asarray(sigma, dtype=np.float64)) ** 2)


def flagged(mask, factor=100.0):
    """s = factor on the flagged rows, 1 elsewhere"""
    return _checked(np.where(np.asarray(mask, dtype=bool), float(factor), 1.0))


def outlier_weight(scale):
    """1 / s: E tau_i, the weight of row i's precision in the posterior mean"""
    return 1.0 / np.asarray(scale, dtype=np.float64)


def _digamma(x):
    """psi(x), x > 0: recurrence up to x >= 12, then the asymptotic series (robust_tables.h has the same)"""
    r = 0.0
    while x < 12.0:
        r -= 1.0 / x
        x += 1.0
    i2 = 1.0 / (x * x)
    ser = i2 * (1.0 / 12 - i2 * (1.0 / 120 - i2 * (1.0 / 252 - i2 * (1.0 / 240 - i2 * (1.0 / 132 - i2 * (691.0 / 32760 - i2 / 12))))))
    return r + ((math.log(x) - 0.5 / x) - ser)


def kappa_const(nu):
    """C(nu) = psi(a) / 2 - lgamma(a) + lgamma(c) + c log(a / c) - a - (psi(a) - log a) / 2,  c = nu / 2,  a = (nu + 1) / 2"""
    nu = float(nu)
    if not (math.isfinite(nu) and nu > 0):
        raise ValueError("nu must be finite and > 0")
    c, a = nu / 2, (nu + 1) / 2
    psi = _digamma(a)
    return ((((psi / 2 - math.lgamma(a)) + math.lgamma(c)) + c * math.log(a / c)) - a) - (psi - math.log(a)) / 2


def dense(K, y, sigma2, nu, sweeps, scale0=None, pi=3.14159265):
    """The robust call in float64 numpy for one patient.  K: the noise-free covariance of the rows [n, n]; sigma2, nu: the noise variance
    and degrees of freedom of every ROW (scalars broadcast); scale0: the starting scales (None: ones); pi: the constant in n log(2 pi) / 2
    (the library's default, medgp_set_pi).  Returns dict(obj, nlml, scale,
    resid, fvar, delta, alpha, trace) with trace[k] = J after k sweeps (non-increasing)."""
    K = np.asarray(K, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    sig2 = np.broadcast_to(np.asarray(sigma2, dtype=np.float64), (n,))
    nur = np.broadcast_to(np.asarray(nu, dtype=np.float64), (n,))
    s = np.ones(n) if scale0 is None else _checked(scale0).copy()
    cst = {v: kappa_const(v) for v in np.unique(nur)}
    csum = math.fsum(cst[v] for v in nur)

    def evaluate(s):
        N = sig2 * s
        L = np.linalg.cholesky(K + np.diag(N))
        Li = np.linalg.solve(L, np.eye(n))
        z = Li @ y
        alpha = Li.T @ z
        pd = np.sum(Li * Li, axis=0)
        nlml = (z @ z) / 2 + np.sum(np.log(np.diagonal(L))) + n * math.log(2 * pi) / 2
        obj = nlml + np.sum((nur / 2) * (np.log(s) + 1 / s)) + csum
        return dict(obj=obj, nlml=nlml, resid=N * alpha, fvar=N - N * N * pd, alpha=alpha)

    trace, delta = [], 0.0
    for _ in range(int(sweeps)):
        r = evaluate(s)
        trace.append(r["obj"])
        sn = (nur + (r["resid"] ** 2 + r["fvar"]) / sig2) / (nur + 1)
        delta = float(np.max(np.abs(sn - s) / sn))
        s = sn
    r = evaluate(s)
    trace.append(r["obj"])
    r.update(scale=s, delta=delta, trace=trace)
    return r


def fit(ctx, slots, theta0, nu, sweeps=2, warm=True):
    """Optimiser closures for training theta under Student-t noise: returns (fun, state).  fun(theta) -> (J [nbatch], grad [nbatch, H],
    status) evaluates ctx.robust_nlml_grad with `sweeps` E-steps, starting (warm=True) from the scales the previous evaluation ended
    with -- a handful of sweeps per evaluation then follows the fixed point as theta moves.  state: dict(scale, delta, evals, theta)
    of the last evaluation, scale None before the first.  theta0 only fixes the shapes and is what state['theta'] starts at."""
    slots = np.ascontiguousarray(slots, dtype=np.int32).ravel()
    state = dict(scale=None, delta=None, evals=0, theta=np.array(theta0, dtype=np.float64))

    def fun(theta):
        r = ctx.robust_nlml_grad(slots, theta, nu, sweeps=sweeps, scale0=state["scale"] if warm else None, rows=False)
        ok = r["status"] >= 0
        if state["scale"] is None or np.all(ok):
            sc = r["scale"]
        else:   # a failed entry keeps the scales it had: its NaN rows would be refused as a start
            sc = [a if good else b for a, b, good in zip(r["scale"], state["scale"], ok)]
        if all(np.all(np.isfinite(a)) for a in sc):
            state["scale"] = [np.clip(a, SCALE_MIN, SCALE_MAX) for a in sc]
        state.update(delta=r["delta"], evals=state["evals"] + 1, theta=np.array(theta, dtype=np.float64))
        return r["obj"], r["grad"], r["status"]
    return fun, state


def select_nu(ctx, slot, theta, grid, sweeps=8):
    """J at every nu of `grid` for the patient in `slot`, in ONE call (the entries share the slot).  grid: [G] (the same nu for every
    covariate) or [G, D].  Returns (J [G], the index of the smallest, status [G])."""
    g = np.asarray(grid, dtype=np.float64)
    G = g.shape[0]
    D = ctx.D if ctx.kernel_index == 7 else 1
    nu = np.broadcast_to(g.reshape(G, -1), (G, D))
    th = np.broadcast_to(np.asarray(theta, dtype=np.float64).reshape(1, -1), (G, ctx.H))
    r = ctx.robust_nlml_grad(np.full(G, int(slot), dtype=np.int32), th, nu, sweeps=sweeps, flag_grad=False, rows=False)
    J = np.where(r["status"] >= 0, r["obj"], np.inf)
    return r["obj"], int(np.argmin(J)), r["status"]


def _t_cdf_grid(nu, x):
    """the Student-t cdf on the sorted grid x by cumulative trapezoid of its density, normalised (numpy only)"""
    lg = math.lgamma((nu + 1) / 2) - math.lgamma(nu / 2) - 0.5 * math.log(nu * math.pi)
    pdf = np.exp(lg - (nu + 1) / 2 * np.log1p(x * x / nu))
    cdf = np.concatenate([[0.0], np.cumsum((pdf[1:] + pdf[:-1]) / 2 * np.diff(x))])
    return pdf, cdf / cdf[-1]


def predictive_interval(mean, var_latent, sigma2, nu, level=0.95, nodes=64):
    """The central `level` interval of a NEW observation y* = f* + eps*: f* ~ N(mean, var_latent) (hetero_posterior with s2 = 0 at the
    scales the robust call ended with) and eps* ~ sigma t_nu, by Gauss-Hermite quadrature over f* and a tabulated t cdf.  Arrays
    broadcast; returns (lo, hi)."""
    mean, vl, s2, nu = np.broadcast_arrays(*[np.asarray(a, dtype=np.float64) for a in (mean, var_latent, sigma2, nu)])
    xg, wg = np.polynomial.hermite_e.hermegauss(nodes)
    wg = wg / wg.sum()
    lo, hi = np.empty(mean.shape), np.empty(mean.shape)
    x = np.concatenate([-np.geomspace(1e6, 1e-4, 3000), [0.0], np.geomspace(1e-4, 1e6, 3000)])
    tables = {}
    a = (1 - level) / 2
    for idx in np.ndindex(mean.shape):
        v = float(nu[idx])
        if v not in tables:
            tables[v] = _t_cdf_grid(v, x)[1]
        cdf = tables[v]
        sd_f, sd_e = math.sqrt(max(vl[idx], 0.0)), math.sqrt(s2[idx])
        span = 12.0 * sd_f + sd_e * 1e3
        ys = mean[idx] + np.concatenate([-np.geomspace(span, 1e-6 * sd_e, 400), [0.0], np.geomspace(1e-6 * sd_e, span, 400)])
        F = np.array([np.dot(wg, np.interp((yv - (mean[idx] + sd_f * xg)) / sd_e, x, cdf)) for yv in ys])
        lo[idx], hi[idx] = np.interp(a, F, ys), np.interp(1 - a, F, ys)
    return lo, hi
