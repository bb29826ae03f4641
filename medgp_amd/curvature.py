"""Second-order tools on the exact Hessian of the marginal likelihood (medgp_hess_vec): the matvec binding, the curvature of the
separable priors, a Newton-CG step that falls back to the Fisher information where the Hessian has no positive curvature, and the
Laplace approximation of the evidence.

The matvec convention is medgp_amd.information's: V [nbatch, nvec, H] -> H V [nbatch, nvec, H], so information.fisher_matrix (the full
matrix from unit directions) and information.solve take a Hessian matvec as they are.  The device Hessian is that of the data term
L = 1/2 y^T K^-1 y + 1/2 log det K alone; prior_curvature gives what the priors add on the diagonal.  All host numpy.
"""
import numpy as np

from . import information


class NotPositiveDefinite(ValueError):
    """laplace_evidence: the Hessian restricted to the free hypers is not positive definite (theta is not a minimum)"""


def bind(ctx, slots, theta):
    """matvec of the exact Hessian of the patients in `slots` at `theta` [nbatch, H] on a capi.Context; a failed patient's products
    are NaN"""
    slots = np.ascontiguousarray(slots, dtype=np.int32)
    theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(slots.shape[0], -1)

    def matvec(V):
        return ctx.hess_vec(slots, theta, V)[0]
    return matvec


def prior_curvature(flag, type, p0, p1, is_exp, theta):
    """(diag, free) of the separable priors the objective calls apply: diag[h] = -d^2 log p_h / d theta_h^2 in THETA space, free[h] =
    False where a clamp (type 0) pins the hyper -- such hypers drop out of rows and columns of a Hessian.  All arguments are arrays
    over the hypers.  A prior is evaluated at x = exp(theta) where is_exp is set (the chain rule then adds log p'(x) x to the second
    derivative) and at x = theta otherwise:
        normal  (type 1, mean p0, variance p1):  x'^2 / p1 + (x - p0) x'' / p1
        Laplace (type 2, location p0, scale p1): sign(x - p0) x'' / p1 -- no curvature of its own away from the kink, and none at it
                                                 (the gradient's convention: slope 0 at x = p0)
    with x' = x'' = x under is_exp and x' = 1, x'' = 0 without.  No prior (flag 0, or another type): 0."""
    flag, type_ = np.asarray(flag).astype(bool), np.asarray(type).astype(np.int64)
    p0, p1 = np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64)
    ex = np.asarray(is_exp).astype(bool)
    th = np.asarray(theta, dtype=np.float64)
    x = np.where(ex, np.exp(th), th)
    x1 = np.where(ex, x, 1.0)
    x2 = np.where(ex, x, 0.0)
    safe = np.where(p1 != 0, p1, 1.0)
    normal = x1 * x1 / safe + (x - p0) * x2 / safe
    laplace = np.sign(x - p0) * x2 / safe
    diag = np.where(flag & (type_ == 1), normal, np.where(flag & (type_ == 2), laplace, 0.0))
    return diag, ~(flag & (type_ == 0))


def newton_step(hess_mv, fisher_mv, g, damping=0.0, tol=1e-10, max_iter=None):
    """x with H x = g by conjugate gradients on the exact Hessian (the Newton step of a minimisation is -x), every patient at once.
    g [nbatch, H].  CG on H is truncated at the first direction p with p (H + damping I) p <= 0: H is indefinite there, and that
    patient falls back to the Fisher information -- positive semi-definite -- for its whole step: x = information.solve(fisher_mv, g,
    damping).  Returns (x [nbatch, H], used_fisher [nbatch] bool, iterations [nbatch], converged [nbatch])."""
    g = np.asarray(g, dtype=np.float64)
    nb, H = g.shape
    max_iter = H if max_iter is None else int(max_iter)
    x = np.zeros_like(g)
    r = g.copy()
    p = r.copy()
    rs = np.einsum("bh,bh->b", r, r)
    gn = np.sqrt(rs)
    done = rs <= (tol * gn) ** 2
    conv = done.copy()
    neg = np.zeros(nb, dtype=bool)
    its = np.zeros(nb, dtype=np.int64)
    for _ in range(max_iter):
        if done.all():
            break
        Ap = np.asarray(hess_mv(p[:, None, :]), dtype=np.float64).reshape(nb, H) + damping * p
        pAp = np.einsum("bh,bh->b", p, Ap)
        bad = ~done & ~(pAp > 0)
        neg = neg | bad
        done = done | bad
        act = ~done
        a = np.where(act, rs / np.where(act, pAp, 1.0), 0.0)
        x = x + a[:, None] * p
        r = r - a[:, None] * Ap
        rs2 = np.einsum("bh,bh->b", r, r)
        its = its + act
        now = act & (np.sqrt(rs2) <= tol * gn)
        conv = conv | now
        done = done | now
        beta = np.where(done, 0.0, rs2 / np.where(rs > 0, rs, 1.0))
        p = np.where(done[:, None], p, r + beta[:, None] * p)
        rs = np.where(done, rs, rs2)
    if neg.any():
        xf, itf, cf = information.solve(fisher_mv, g, damping=damping, tol=tol, max_iter=max_iter)
        x = np.where(neg[:, None], xf, x)
        its = np.where(neg, itf, its)
        conv = np.where(neg, cf, conv)
    return x, neg, its, conv


def laplace_evidence(nlml_post, Hfull, free=None):
    """log evidence of one patient by the Laplace approximation at a posterior mode:
        -nlml_post + |free| / 2 log 2 pi - 1/2 log det H[free, free]
    nlml_post: the objective at the mode (negative log likelihood minus log prior); Hfull [H, H]: its Hessian there (the device
    Hessian plus prior_curvature's diagonal); free: bool mask or indices of the hypers that vary (default all).  Raises
    NotPositiveDefinite when the restricted Hessian is not positive definite: theta is then no minimum and the approximation has
    no value."""
    Hm = np.asarray(Hfull, dtype=np.float64)
    Hm = (Hm + Hm.T) / 2
    idx = np.arange(Hm.shape[0]) if free is None else np.asarray(free)
    if idx.dtype == bool:
        idx = np.flatnonzero(idx)
    Hf = Hm[np.ix_(idx, idx)]
    k = idx.shape[0]
    if k == 0:
        return -float(nlml_post)
    w = np.linalg.eigvalsh(Hf)
    if not np.isfinite(w).all() or not w[0] > 0:
        raise NotPositiveDefinite(f"smallest eigenvalue {w[0]:.3g} of the Hessian on the {k} free hypers: not a minimum")
    return -float(nlml_post) + 0.5 * k * np.log(2 * np.pi) - 0.5 * float(np.sum(np.log(w)))
