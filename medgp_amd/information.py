"""Curvature of the marginal likelihood from Fisher-information products (medgp_fisher_vec): a patient's full Fisher matrix for small
H, the natural-gradient / Fisher-scoring step by conjugate gradients, Cramer-Rao standard errors of trained hypers, and the direction
along which all amplitudes grow together.

Every helper takes a `matvec` callable, V [nbatch, nvec, H] -> F V [nbatch, nvec, H] (patient b's F applied to each of its nvec
directions), so that it can be tested without a GPU; `bind(ctx, slots, theta)` makes that callable from a Context.  F is the
information of the likelihood alone (no prior) at the theta the callable was bound to.
"""
import numpy as np


def bind(ctx, slots, theta):
    """matvec of the patients in `slots` at `theta` [nbatch, H] on a capi.Context; a failed patient's products are NaN"""
    slots = np.ascontiguousarray(slots, dtype=np.int32)
    theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(slots.shape[0], -1)

    def matvec(V):
        return ctx.fisher_vec(slots, theta, V)[0]
    return matvec


def fisher_matrix(matvec, H, free=None, nbatch=1):
    """F restricted to the hypers `free` (indices, default all), symmetrised: [nbatch, |free|, |free|], from ONE call of matvec with the
    |free| unit directions of every patient"""
    free = np.arange(H) if free is None else np.asarray(free, dtype=np.int64)
    k = free.shape[0]
    V = np.zeros((nbatch, k, H))
    V[:, np.arange(k), free] = 1.0
    FV = np.asarray(matvec(V), dtype=np.float64).reshape(nbatch, k, H)
    F = FV[:, :, free]
    return (F + F.transpose(0, 2, 1)) / 2


def solve(matvec, g, damping=0.0, tol=1e-10, max_iter=None):
    """Conjugate gradients on (F + damping I) x = g for every patient at once: the natural-gradient / Fisher-scoring step F^-1 g.
    g [nbatch, H].  A patient stops on its own flag, ||r|| <= tol ||g|| (or on a direction of no curvature, p (F + damping I) p <= 0:
    F is only positive SEMI-definite), and keeps its x from then on; the loop ends when all have stopped or after max_iter (default H)
    products.  Returns (x [nbatch, H], iterations [nbatch], converged [nbatch])."""
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
    its = np.zeros(nb, dtype=np.int64)
    for _ in range(max_iter):
        if done.all():
            break
        Ap = np.asarray(matvec(p[:, None, :]), dtype=np.float64).reshape(nb, H) + damping * p
        pAp = np.einsum("bh,bh->b", p, Ap)
        flat = ~done & ~(pAp > 0)          # no curvature along p (or NaN: a failed patient): nothing more to gain
        done = done | flat
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
    return x, its, conv


def stderr(F, rcond=None):
    """Cramer-Rao bound on the free hypers of one patient: sqrt(diag(pinv(F))) and the rank used.  Eigenvalues at or below
    rcond * largest (default |free| * eps) count as zero.  The pseudo-inverse gives 0, not infinity, to a hyper the data do not
    determine at all (an exact zero row, as of a covariate without observations): read the figures together with the rank, or
    leave such hypers out of `free`."""
    F = np.asarray(F, dtype=np.float64)
    F = (F + F.T) / 2
    k = F.shape[0]
    se = np.zeros(k)
    live = np.flatnonzero(np.abs(F).sum(axis=1) > 0)      # exact zero rows are decoupled: they stay exact zeros of the pseudo-inverse
    if live.size == 0:
        return se, 0
    w, U = np.linalg.eigh(F[np.ix_(live, live)])
    rc = k * np.finfo(np.float64).eps if rcond is None else rcond
    keep = w > rc * max(float(w[-1]), 0.0)
    rank = int(keep.sum())
    var = np.einsum("ij,j,ij->i", U[:, keep], 1.0 / w[keep], U[:, keep])
    se[live] = np.sqrt(np.maximum(var, 0.0))
    return se, rank


def scale_direction(kidx, Q, D, R, theta):
    """The direction s in theta space along which every amplitude grows together, Kdot = 2 K (so F s = grad_from_w(2 P) and
    s^T F s = 2 n).  LMC-SM: 1 on log sigma, A itself on the A block, 0 on log mu / log v, 2 on log kappa.  SM: 1 on log sigma, 2 on
    log w.  SE: 1 on log sigma and log sf."""
    th = np.asarray(theta, dtype=np.float64)
    s = np.zeros_like(th)
    if kidx == 7:
        s[:D] = 1.0
        s[D:D + Q * D * R] = th[D:D + Q * D * R]
        s[D + Q * (D * R + 2):] = 2.0
    elif kidx == 8:
        s[0] = 1.0
        s[1:1 + Q] = 2.0
    elif kidx == 0:
        s[0] = 1.0
        s[2] = 1.0
    else:
        raise ValueError(kidx)
    return s
