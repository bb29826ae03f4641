"""Training on a predictive score on medgp_posterior_vjp_batch (capi.Context.posterior_vjp): the gradient over all hypers of any
scalar loss of the posterior mean and variance at held-out points, from one factorisation per patient.

    nlpd, sqerr, crps            numpy restatements of the device's built-in losses: (value, dloss/dmean, dloss/dvar)
    pinball(tau), interval_score(alpha)   further losses of a normal forecast, as examples of custom cotangents
    loss_and_grad                one call for a built-in loss; a call for the fp64 mean / var plus a custom VJP call for a callable
    jacobian_rows                rows of the Jacobians of mean and var for a few points (the cotangent sets of ONE call)
    TorchPosterior               torch.autograd.Function: loss(mean, var).backward() fills theta.grad

All host numpy / torch around the device calls; the per-point arrays are float64.
"""
import math

import numpy as np

_erf = np.vectorize(math.erf, otypes=[np.float64])
_SQRT_PI = math.sqrt(math.pi)


def _arr(*xs):
    X = np.result_type(np.float64, *[np.asarray(x).dtype for x in xs])
    return [np.asarray(x, dtype=X) for x in xs]


def _phi_terms(z):
    """(2 Phi(z) - 1, phi(z)) of the standard normal; erf in float64 (the arguments keep their own precision elsewhere)"""
    e2 = _erf(np.asarray(z, np.float64) / math.sqrt(2.0)).astype(z.dtype)
    return e2, np.exp(-z * z / 2) / np.sqrt(2 * z.dtype.type(np.pi))


def nlpd(mean, var, y, wt=None):
    """sum_j wt_j (1/2 log(2 pi var_j) + (y_j - mean_j)^2 / (2 var_j)) with its derivatives in mean and var"""
    mean, var, y = _arr(mean, var, y)
    w = np.ones_like(mean) if wt is None else np.asarray(wt, mean.dtype)
    r = y - mean
    l = np.log(2 * mean.dtype.type(np.pi) * var) / 2 + r * r / (2 * var)
    return np.sum(w * l), -w * r / var, w * (1 / (2 * var) - r * r / (2 * var * var))


def sqerr(mean, var, y, wt=None):
    """sum_j wt_j (y_j - mean_j)^2"""
    mean, var, y = _arr(mean, var, y)
    w = np.ones_like(mean) if wt is None else np.asarray(wt, mean.dtype)
    r = y - mean
    return np.sum(w * r * r), -2 * w * r, np.zeros_like(mean)


def crps(mean, var, y, wt=None):
    """the continuous ranked probability score of the normal forecasts: s (z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi)), z = (y - mean) / s"""
    mean, var, y = _arr(mean, var, y)
    w = np.ones_like(mean) if wt is None else np.asarray(wt, mean.dtype)
    s = np.sqrt(var)
    z = (y - mean) / s
    e2, phi = _phi_terms(z)
    c = 2 * phi - 1 / mean.dtype.type(_SQRT_PI)
    return np.sum(w * s * (z * e2 + c)), -w * e2, w * c / (2 * s)


BUILTIN = {"nlpd": nlpd, "sqerr": sqerr, "crps": crps}


def _norm_ppf(p):
    """the standard normal quantile by Newton steps on erf (no scipy): p in (0, 1)"""
    x = 0.0
    for _ in range(60):
        f = 0.5 * (1.0 + math.erf(x / math.sqrt(2.0))) - p
        x -= f / (math.exp(-x * x / 2) / math.sqrt(2 * math.pi))
    return x


def pinball(tau):
    """The pinball loss of the forecast's tau-quantile q = mean + z_tau sqrt(var): loss(mean, var, y) -> (value, cot_mean, cot_var).
    Piecewise linear in q: the cotangents are those of the active piece."""
    zt = _norm_ppf(float(tau))

    def f(mean, var, y, wt=None):
        mean, var, y = _arr(mean, var, y)
        w = np.ones_like(mean) if wt is None else np.asarray(wt, mean.dtype)
        s = np.sqrt(var)
        d = y - (mean + zt * s)
        dq = np.where(d >= 0, -tau, 1 - tau)           # dloss / dq
        return np.sum(w * np.where(d >= 0, tau * d, (tau - 1) * d)), w * dq, w * dq * zt / (2 * s)
    return f


def interval_score(alpha):
    """The interval score of the central 1 - alpha interval [l, u] = mean -+ z sqrt(var): (u - l) + 2 / alpha ((l - y)+ + (y - u)+)"""
    z = _norm_ppf(1.0 - float(alpha) / 2)

    def f(mean, var, y, wt=None):
        mean, var, y = _arr(mean, var, y)
        w = np.ones_like(mean) if wt is None else np.asarray(wt, mean.dtype)
        s = np.sqrt(var)
        lo, up = mean - z * s, mean + z * s
        below, above = y < lo, y > up
        val = (up - lo) + (2 / alpha) * (np.where(below, lo - y, 0) + np.where(above, y - up, 0))
        dlo = -1 + (2 / alpha) * below                   # dloss / dl
        dup = 1 - (2 / alpha) * above                    # dloss / du
        return np.sum(w * val), w * (dlo + dup), w * (dup - dlo) * z / (2 * s)
    return f


def loss_and_grad(ctx, slots, theta, meta2_list, t2_list, y2_list, loss="nlpd", wt_list=None):
    """([(value, grad[H]) per patient], status).  loss: "nlpd" | "sqerr" | "crps" (ONE device call: the device forms the cotangents
    from its own fp64 mean and var) or a callable loss(mean, var, y, wt) -> (value, cot_mean, cot_var) such as pinball(0.9) (a
    first call for the fp64 mean and var, then a custom VJP call)."""
    if isinstance(loss, str):
        out, st = ctx.posterior_vjp(slots, theta, meta2_list, t2_list, loss=loss, y2_list=y2_list, wt_list=wt_list, want_posterior=False)
        return [(o[3], o[2]) for o in out], st
    zeros = [np.zeros(np.size(x)) for x in t2_list]
    post, st = ctx.posterior_vjp(slots, theta, meta2_list, t2_list, cot_mean=zeros, cot_var=zeros, fp64_posterior=True)
    vals, cms, cvs = [], [], []
    for b, pp in enumerate(post):
        v, cm, cv = loss(np.asarray(pp[0], np.float64), np.asarray(pp[1], np.float64), np.asarray(y2_list[b], np.float64),
                         None if wt_list is None else np.asarray(wt_list[b], np.float64))
        vals.append(float(v)); cms.append(cm); cvs.append(cv)
    out, st = ctx.posterior_vjp(slots, theta, meta2_list, t2_list, cot_mean=cms, cot_var=cvs, want_posterior=False)
    return [(vals[b], out[b][2][0]) for b in range(len(out))], st


def jacobian_rows(ctx, slots, theta, meta2_list, t2_list, points):
    """Rows of the Jacobians of mean and var: points = one index array per patient (into its test points, the same number r for
    all).  ONE device call with 2 r cotangent sets.  Returns ([(Jmean[r, H], Jvar[r, H]) per patient], status) -- cheaper than H JVP
    directions when r is small against H."""
    pts = [np.asarray(p, dtype=np.int64).ravel() for p in points]
    r = pts[0].shape[0]
    if any(p.shape[0] != r for p in pts) or r < 1:
        raise ValueError("the same number (>= 1) of points for every patient")
    cms, cvs = [], []
    for b, p in enumerate(pts):
        m = np.size(t2_list[b])
        if p.size and (p.min() < 0 or p.max() >= m):
            raise ValueError(f"patient {b}: point index outside [0, {m})")
        cm, cv = np.zeros((m, 2 * r)), np.zeros((m, 2 * r))
        cm[p, np.arange(r)] = 1.0
        cv[p, r + np.arange(r)] = 1.0
        cms.append(cm); cvs.append(cv)
    out, st = ctx.posterior_vjp(slots, theta, meta2_list, t2_list, cot_mean=cms, cot_var=cvs, want_posterior=False)
    return [(o[2][:r].copy(), o[2][r:].copy()) for o in out], st


def _torch_posterior():
    import torch

    class TorchPosterior(torch.autograd.Function):
        """mean, var = TorchPosterior.apply(theta, ctx, slots, meta2_list, t2_list): the plug-in posterior of every point of the call
        as CPU float64 tensors [M] (patients concatenated; the device's fp64 values, not its float outputs); theta [nbatch, H] CPU
        float64.  backward runs the custom VJP call, so
        loss(mean, var).backward() fills theta.grad."""

        @staticmethod
        def forward(fctx, theta, ctx, slots, meta2_list, t2_list):
            th = theta.detach().cpu().double().numpy()
            cnt = [int(np.size(x)) for x in t2_list]
            zeros = [np.zeros(m) for m in cnt]
            out, st = ctx.posterior_vjp(slots, th, meta2_list, t2_list, cot_mean=zeros, cot_var=zeros, want_posterior=True, fp64_posterior=True)
            fctx.call = (ctx, slots, th, meta2_list, t2_list, cnt)
            mean = np.concatenate([o[0] for o in out]).astype(np.float64) if sum(cnt) else np.zeros(0)
            var = np.concatenate([o[1] for o in out]).astype(np.float64) if sum(cnt) else np.zeros(0)
            return torch.from_numpy(mean), torch.from_numpy(var)

        @staticmethod
        def backward(fctx, gmean, gvar):
            ctx, slots, th, meta2_list, t2_list, cnt = fctx.call
            off = np.concatenate([[0], np.cumsum(cnt)])
            gm = np.zeros(int(off[-1])) if gmean is None else gmean.detach().double().numpy()
            gv = np.zeros(int(off[-1])) if gvar is None else gvar.detach().double().numpy()
            cms = [gm[off[b]:off[b + 1]] for b in range(len(cnt))]
            cvs = [gv[off[b]:off[b + 1]] for b in range(len(cnt))]
            out, _ = ctx.posterior_vjp(slots, th, meta2_list, t2_list, cot_mean=cms, cot_var=cvs, want_posterior=False)
            g = np.stack([o[2][0] for o in out])
            return torch.from_numpy(g), None, None, None, None

    return TorchPosterior


def __getattr__(name):
    if name == "TorchPosterior":   # built on first use: importing this module does not import torch
        cls = _torch_posterior()
        globals()["TorchPosterior"] = cls
        return cls
    raise AttributeError(name)
