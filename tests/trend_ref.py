"""numpy definition of medgp_trend_batch: the posterior of the latent slope f'_{m*}(t*) at the test points, next to the posterior
of the value.  The reference program has no such output, so this file IS the definition (include/medgp_hip.h).

Component q is k_q(tau) = cos(w_q tau) exp(-c_q tau^2), w_q = 2 PI mu_q, c_q = 2 (PI v_q)^2 (SE: w = 0, c = 1 / (2 l^2), B = sf^2),
with the reference's PI and the coregionalisation matrices B_q of the oracle.  For tau = t* - t_i:
    K*[i]   = sum_q B_q[m_i, m*] cos(w_q tau) exp(-c_q tau^2)
    K*'[i]  = sum_q B_q[m_i, m*] (-w_q sin(w_q tau) - 2 c_q tau cos(w_q tau)) exp(-c_q tau^2)        (d/dt* of K*[i])
    k''**   = sum_q B_q[m*, m*] (w_q^2 + 2 c_q)                                                     (-k''(0): prior variance of f')
    V = L^-1 K*,  V' = L^-1 K*',  z = L^-1 y,   L L^T = K + (1 + jitter_rounds) diag(sigma^2)
    mean = V^T z,  var = k** - sum V^2 + sigma^2_{m*},  dmean = V'^T z,  dvar = k''** - sum V'^2,  cross = - sum V V'.
restate() writes this down twice: in fp64 on numpy's LAPACK, and (dtype=np.longdouble) with its own Cholesky and forward solves, as
the truth the fp64 one is held to (test_trend.py).  check_trend() is the bound the GPU tests hold the device outputs to."""
import numpy as np

from oracle import oracle as O
import posterior_ref as PR

NAMES = ("mean", "var", "dmean", "dvar", "cross")


def hypers(kidx, Q, D, R, theta, dtype=np.float64, pi=O.REF_PI):
    """(sigma^2 [D'], B [Q, D', D'], w [Q], c [Q]) as k_prep leaves them in the hyp block; D' = 1 for SE / SM"""
    th = np.asarray(theta, np.float64)
    thx = th.astype(dtype)
    pi = dtype(pi)
    if kidx == O.KERNEL_LMC_SM:
        sig2 = np.exp(thx[:D]) ** 2
        B = O.coregional(Q, D, R, th[D:]).astype(dtype)
        o = D + Q * D * R
        mu, v = np.exp(thx[o:o + Q]), np.exp(thx[o + Q:o + 2 * Q])
    elif kidx == O.KERNEL_SM:    # theta = [log sigma | log weight | log mu | log v]
        sig2 = np.exp(thx[:1]) ** 2
        B = np.exp(thx[1:1 + Q]).reshape(Q, 1, 1)
        mu, v = np.exp(thx[1 + Q:1 + 2 * Q]), np.exp(thx[1 + 2 * Q:1 + 3 * Q])
    elif kidx == O.KERNEL_SE:    # theta = [log sigma | log l | log sf]
        assert Q == 1
        sig2 = np.exp(thx[:1]) ** 2
        ell, sf = np.exp(thx[1]), np.exp(thx[2])
        return sig2, (sf * sf).reshape(1, 1, 1), np.zeros(1, dtype), (dtype(0.5) / (ell * ell)).reshape(1)
    else:
        raise ValueError(kidx)
    return sig2, B, dtype(2) * pi * mu, dtype(2) * (pi * v) ** 2


def _chol(A):
    """lower Cholesky factor, column by column, in A's dtype (numpy's LAPACK has no long double)"""
    n = A.shape[0]
    Lc = np.zeros_like(A)
    for j in range(n):
        col = A[j:, j] - Lc[j:, :j] @ Lc[j, :j]
        assert col[0] > 0, "not positive definite"
        Lc[j:, j] = col / np.sqrt(col[0])
    return Lc


def _fsolve(Lc, Bm):
    """Lc^-1 Bm by forward substitution in Lc's dtype"""
    X = np.zeros_like(Bm)
    for i in range(Lc.shape[0]):
        X[i] = (Bm[i] - Lc[i, :i] @ X[:i]) / Lc[i, i]
    return X


def _gram(B, w, c, ma, ta, mb, tb, slope=False):
    """K[i, j] = sum_q B_q[ma_i, mb_j] k_q(tb_j - ta_i), and with slope=True also its derivative in tb_j"""
    dtype = ta.dtype.type
    tau = tb[None, :] - ta[:, None]
    K = np.zeros(tau.shape, dtype)
    Kd = np.zeros(tau.shape, dtype) if slope else None
    for q in range(B.shape[0]):
        Bs = B[q][ma[:, None], mb[None, :]]
        e = np.exp(-c[q] * tau * tau)
        co = np.cos(w[q] * tau)
        K += Bs * (co * e)
        if slope:
            Kd += Bs * ((-w[q] * np.sin(w[q] * tau) - dtype(2) * c[q] * tau * co) * e)
    return (K, Kd) if slope else K


def _factor(Kxx):
    return np.linalg.cholesky(Kxx) if Kxx.dtype == np.float64 else _chol(Kxx)


def _solve(Lc, Bm):
    return np.linalg.solve(Lc, Bm) if Lc.dtype == np.float64 else _fsolve(Lc, Bm)


def _train(kidx, Q, D, R, meta, t, theta, jitter_rounds, dtype):
    """(sigma^2, B, w, c, meta, t, L) of the training set in dtype"""
    t = np.asarray(t, np.float32).astype(dtype)
    n = t.shape[0]
    meta = np.asarray(meta, np.int64) if kidx == O.KERNEL_LMC_SM else np.zeros(n, np.int64)
    sig2, B, w, c = hypers(kidx, Q, D, R, theta, dtype)
    Kxx = _gram(B, w, c, meta, t, meta, t)
    Kxx[np.diag_indices(n)] += dtype(1 + jitter_rounds) * sig2[meta]
    return sig2, B, w, c, meta, t, _factor(Kxx)


def restate(kidx, Q, D, R, meta, t, y, theta, meta2, t2, jitter_rounds=0, dtype=np.float64):
    """Returns (mean[m], var[m], dmean[m], dvar[m], cross[m], prior_dvar[m]) in dtype.  meta / meta2 are ignored for SE / SM (may be
    None).  jitter_rounds = k: every quantity is that of the factor of K + k diag(sigma^2) that k retries leave; var still
    carries the noise of the test covariate once."""
    sig2, B, w, c, meta, t, Lc = _train(kidx, Q, D, R, meta, t, theta, jitter_rounds, dtype)
    t2 = np.asarray(t2, np.float32).astype(dtype)
    yy = np.asarray(y, np.float32).astype(dtype)
    m = t2.shape[0]
    meta2 = np.asarray(meta2, np.int64) if kidx == O.KERNEL_LMC_SM else np.zeros(m, np.int64)
    Ks, Kd = _gram(B, w, c, meta, t, meta2, t2, slope=True)
    kss = np.zeros(m, dtype)
    prior = np.zeros(m, dtype)
    for q in range(Q):
        bss = B[q][meta2, meta2]
        kss += bss
        prior += bss * (w[q] * w[q] + dtype(2) * c[q])
    VV = _solve(Lc, np.concatenate([Ks, Kd, yy[:, None]], axis=1))
    V, Vd, z = VV[:, :m], VV[:, m:2 * m], VV[:, 2 * m]
    mean = V.T @ z
    var = kss - np.sum(V * V, axis=0) + sig2[meta2]
    dmean = Vd.T @ z
    dvar = prior - np.sum(Vd * Vd, axis=0)
    cross = -np.sum(V * Vd, axis=0)
    return mean, var, dmean, dvar, cross, prior


def latent_cov(kidx, Q, D, R, meta, t, theta, meta_a, t_a, meta_b, t_b, dtype=np.longdouble):
    """diag of the posterior covariance cov(f(a_j), f(b_j)) of the LATENT function between paired points a_j, b_j (no noise):
    k(a_j, b_j) - V_a[:, j] . V_b[:, j].  What the finite differences of test_trend.py are taken of."""
    _, B, w, c, meta, t, Lc = _train(kidx, Q, D, R, meta, t, theta, 0, dtype)
    t_a = np.asarray(t_a, np.float32).astype(dtype)
    t_b = np.asarray(t_b, np.float32).astype(dtype)
    m = t_a.shape[0]
    multi = kidx == O.KERNEL_LMC_SM
    meta_a = np.asarray(meta_a, np.int64) if multi else np.zeros(m, np.int64)
    meta_b = np.asarray(meta_b, np.int64) if multi else np.zeros(m, np.int64)
    VV = _solve(Lc, np.concatenate([_gram(B, w, c, meta, t, meta_a, t_a), _gram(B, w, c, meta, t, meta_b, t_b)], axis=1))
    kab = np.zeros(m, dtype)
    tau = t_b - t_a
    for q in range(Q):
        kab += B[q][meta_a, meta_b] * (np.cos(w[q] * tau) * np.exp(-c[q] * tau * tau))
    return kab - np.sum(VV[:, :m] * VV[:, m:], axis=0)


def ulps(dev, ref):
    """the error of each of the five quantities in fp32 ulps of max(|ref|, 1e-3 S) (posterior_ref.ulp_error)"""
    return tuple(PR.ulp_error(d, r) for d, r in zip(dev[:5], ref[:5]))


def check_trend(kidx, D, theta, meta2, ref, out):
    """One patient's device output (mean, var, dmean, dvar, cross or None) against ref = restate(...): every element of every
    quantity within two fp32 ulps of max(|ref|, 1e-3 S), S = the patient's largest |ref| of that quantity (the project's bar,
    posterior_ref.assert_fp32_close), and
        0 <= dvar <= k''** (1 + 2^-22)                             a variance, never above the prior's
        cross^2 <= (var - sigma^2_{m*}) dvar (1 + 1e-5) + tiny      Cauchy-Schwarz of the posterior of (f, f')
    tiny = 2^-21 var dvar + 1e-30: var is an fp32 number that carries sigma^2, so var - sigma^2 is known to one fp32 ulp of var
    (2^-23 var) only, doubled for the rounding of the float product.  Returns the five errors in ulps (cross: 0.0 when None)."""
    m = ref[0].shape[0]
    for k in range(5):
        if out[k] is None:
            assert k == 4
            continue
        assert out[k].shape == (m,) and out[k].dtype == np.float32, (NAMES[k], out[k].shape, out[k].dtype)
    if m == 0:
        return (0.0,) * 5
    for k in range(5):
        if out[k] is not None:
            PR.assert_fp32_close(out[k], np.asarray(ref[k], np.float64), NAMES[k])
    multi = kidx == O.KERNEL_LMC_SM
    sig2 = PR.noise_var(kidx, D, theta, meta2 if multi else np.zeros(m, np.int32))
    var, dvar = out[1].astype(np.float64), out[3].astype(np.float64)
    prior = np.asarray(ref[5], np.float64)
    assert np.all(dvar >= 0.0), "negative slope variance"
    assert np.all(dvar <= prior * (1.0 + 2.0 ** -22)), "slope variance above the prior's"
    if out[4] is not None:
        cr = out[4].astype(np.float64)
        lat = np.maximum(var - sig2, 0.0)
        assert np.all(cr * cr <= lat * dvar * (1.0 + 1e-5) + 2.0 ** -21 * var * dvar + 1e-30), "cross beyond Cauchy-Schwarz"
    return tuple(PR.ulp_error(out[k], np.asarray(ref[k], np.float64)) if out[k] is not None else 0.0 for k in range(5))
