"""Hyper-sensitivity of predictions on medgp_posterior_jvp_batch (capi.Context.posterior_jvp): Jacobians of the posterior mean and
variance in the hypers, a low-rank factor of the hyper covariance from a Hessian (medgp_amd.curvature / information), the
delta-method (Laplace) predictive variance

    var_total = var + sum_r (dmean . s_r)^2,     Sigma_theta ~ S S^T,  s_r the columns of S,

and the sensitivity of a prediction to each hyper group.  All host numpy around one device call per use.
"""
import numpy as np

from .curvature import NotPositiveDefinite

KERNEL_SE, KERNEL_LMC_SM, KERNEL_SM = 0, 7, 8


def jacobian(ctx, slots, theta, meta2_list, t2_list, cols=None, chunk=32):
    """The Jacobians of mean and var in theta by unit directions: [(Jmean[m, |cols|], Jvar[m, |cols|]) per patient] and the status.
    cols: the hypers wanted (indices; default all H -- for small H or a chosen subset: one direction each); chunk: directions per
    device call."""
    slots = np.ascontiguousarray(slots, dtype=np.int32)
    nb = slots.shape[0]
    cols = np.arange(ctx.H) if cols is None else np.asarray(cols, dtype=np.int64).ravel()
    if cols.size and (cols.min() < 0 or cols.max() >= ctx.H):
        raise ValueError(f"cols outside [0, {ctx.H})")
    counts = [np.size(x) for x in t2_list]
    Jm = [np.zeros((m, cols.shape[0])) for m in counts]
    Jv = [np.zeros((m, cols.shape[0])) for m in counts]
    status = np.zeros(nb, dtype=np.int32)
    for a in range(0, cols.shape[0], max(int(chunk), 1)):
        cc = cols[a:a + max(int(chunk), 1)]
        V = np.zeros((nb, cc.shape[0], ctx.H))
        V[:, np.arange(cc.shape[0]), cc] = 1.0
        out, status = ctx.posterior_jvp(slots, theta, meta2_list, t2_list, V, want_posterior=False)
        for b in range(nb):
            Jm[b][:, a:a + cc.shape[0]] = out[b][2]
            Jv[b][:, a:a + cc.shape[0]] = out[b][3]
    return list(zip(Jm, Jv)), status


def covariance_factor(Hfull, free=None, rank=None):
    """S [H, r] with S S^T ~ (H[free, free])^-1 on the free hypers and zero rows elsewhere: the top `rank` directions of the hyper
    covariance (the smallest eigenvalues of the Hessian; default all of the free ones).  Hfull: the Hessian of the objective at the
    mode (the device Hessian plus curvature.prior_curvature's diagonal), free: bool mask or indices.  Raises NotPositiveDefinite
    where curvature.laplace_evidence would: the restricted Hessian is not positive definite, theta is no minimum."""
    Hm = np.asarray(Hfull, dtype=np.float64)
    Hm = (Hm + Hm.T) / 2
    idx = np.arange(Hm.shape[0]) if free is None else np.asarray(free)
    if idx.dtype == bool:
        idx = np.flatnonzero(idx)
    k = idx.shape[0]
    r = k if rank is None else min(int(rank), k)
    S = np.zeros((Hm.shape[0], r))
    if k == 0 or r <= 0:
        return S[:, :max(r, 0)]
    w, U = np.linalg.eigh(Hm[np.ix_(idx, idx)])
    if not np.isfinite(w).all() or not w[0] > 0:
        raise NotPositiveDefinite(f"smallest eigenvalue {w[0]:.3g} of the Hessian on the {k} free hypers: not a minimum")
    S[idx] = U[:, :r] / np.sqrt(w[:r])          # ascending eigenvalues of H: descending variances
    return S


def hyper_variance(dmean):
    """sum_r dmean[:, r]^2: the variance the hyper uncertainty adds to the mean, dmean [m, rank] the JVPs along the columns of S"""
    d = np.asarray(dmean, dtype=np.float64)
    return np.sum(d * d, axis=1)


def laplace_predict(ctx, slots, theta, meta2_list, t2_list, S):
    """The delta-method predictive variance from ONE device call with the columns of S as directions.  S: [H, r] (shared by the
    patients) or [nbatch, H, r].  Returns ([dict(mean, var, var_hyper, var_total) per patient], status): var is the plug-in
    variance, var_total = var + var_hyper."""
    slots = np.ascontiguousarray(slots, dtype=np.int32)
    nb = slots.shape[0]
    S = np.asarray(S, dtype=np.float64)
    if S.ndim == 2:
        S = np.broadcast_to(S, (nb,) + S.shape)
    if S.ndim != 3 or S.shape[0] != nb or S.shape[1] != ctx.H or S.shape[2] < 1:
        raise ValueError(f"S of shape {S.shape} for {nb} patients of {ctx.H} hypers")
    V = np.ascontiguousarray(np.transpose(S, (0, 2, 1)))
    out, status = ctx.posterior_jvp(slots, theta, meta2_list, t2_list, V, want_posterior=True)
    res = []
    for mean, var, dmean, _ in out:
        vh = hyper_variance(dmean)
        res.append(dict(mean=mean, var=var, var_hyper=vh, var_total=var.astype(np.float64) + vh))
    return res, status


def groups(kernel_index, Q, D, R):
    """the hyper groups of a family in theta order: [(name, slice)]"""
    if kernel_index == KERNEL_LMC_SM:
        o = [0, D, D + Q * D * R, D + Q * D * R + Q, D + Q * D * R + 2 * Q, D + Q * (D * R + 2) + Q * D]
        names = ["noise", "A", "mu", "v", "kappa"]
    elif kernel_index == KERNEL_SM:
        o = [0, 1, 1 + Q, 1 + 2 * Q, 1 + 3 * Q]
        names = ["noise", "w", "mu", "v"]
    elif kernel_index == KERNEL_SE:
        o = [0, 1, 2, 3]
        names = ["noise", "l", "sf"]
    else:
        raise ValueError(kernel_index)
    return [(n, slice(a, b)) for n, a, b in zip(names, o[:-1], o[1:])]


def by_group(kernel_index, Q, D, R, Jmean):
    """RMS sensitivity per hyper group: {name: rms[m]} of a full Jacobian Jmean [m, H] (noise, A, mu, v, kappa for LMC-SM; noise, w,
    mu, v for SM; noise, l, sf for SE), rms over the group's hypers"""
    J = np.asarray(Jmean, dtype=np.float64)
    gs = groups(kernel_index, Q, D, R)
    if J.ndim != 2 or J.shape[1] != gs[-1][1].stop:
        raise ValueError(f"Jacobian of shape {J.shape} for {gs[-1][1].stop} hypers")
    return {n: np.sqrt(np.mean(J[:, s] ** 2, axis=1)) for n, s in gs}
