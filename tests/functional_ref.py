"""numpy definition of medgp_functional_batch: the posterior of linear functionals g = sum_k a_k f_{m_k}(t_k) of the latent function.
The reference program has no such output, so this file IS the definition (include/medgp_hip.h).

Component q is k_q(tau) = cos(w_q tau) exp(-c_q tau^2) with w_q, c_q and B_q as k_prep leaves them (trend_ref.hypers).  For a functional
with the terms (m_k, t_k, a_k) and a training observation i = (m_i, t_i), tau = t_k - t_i:
    K*_g[i] = sum_k a_k sum_q B_q[m_i, m_k] k_q(tau)
    V_g = L^-1 K*_g,  z = L^-1 y,   L L^T = K + (1 + jitter_rounds) diag(sigma^2)
    fmean = V_g^T z
    q_g   = sum_kl a_k a_l sum_q B_q[m_k, m_l] k_q(t_k - t_l)            the prior variance of g
    fvar  = q_g - V_g^T V_g                                              (latent: no sigma^2)
restate() writes this down twice: in fp64 on numpy's LAPACK, and (dtype=np.longdouble) with trend_ref's own Cholesky and forward
solves, as the truth the fp64 one is held to (test_functional.py).  check_functional() is the bound the GPU tests hold the device
outputs to."""
import numpy as np

from oracle import oracle as O
import posterior_ref as PR
import trend_ref as TR

NAMES = ("fmean", "fvar")


def restate(kidx, Q, D, R, meta, t, y, theta, toffsets, meta2, t2, weight, jitter_rounds=0, dtype=np.float64):
    """Returns (fmean[F], fvar[F], q_g[F]) in dtype for the F = len(toffsets) - 1 functionals whose terms are
    [toffsets[f], toffsets[f + 1]) of meta2 / t2 / weight.  meta / meta2 are ignored for SE / SM (may be None).  jitter_rounds = k:
    every quantity is that of the factor of K + k diag(sigma^2) that k retries leave."""
    sig2, B, w, c, meta, t, Lc = TR._train(kidx, Q, D, R, meta, t, theta, jitter_rounds, dtype)
    toff = np.asarray(toffsets, np.int64)
    t2 = np.asarray(t2, np.float32).astype(dtype)
    a = np.asarray(weight, np.float64).astype(dtype)
    yy = np.asarray(y, np.float32).astype(dtype)
    n, T, F = t.shape[0], t2.shape[0], toff.shape[0] - 1
    assert toff[0] == 0 and toff[-1] == T == a.shape[0]
    meta2 = np.asarray(meta2, np.int64) if kidx == O.KERNEL_LMC_SM else np.zeros(T, np.int64)
    Ks = TR._gram(B, w, c, meta, t, meta2, t2)                                  # [n, T]
    Kg = np.zeros((n, F), dtype)
    qg = np.zeros(F, dtype)
    for f in range(F):
        s = slice(int(toff[f]), int(toff[f + 1]))
        Kg[:, f] = Ks[:, s] @ a[s]
        qg[f] = a[s] @ (TR._gram(B, w, c, meta2[s], t2[s], meta2[s], t2[s]) @ a[s])
    VV = TR._solve(Lc, np.concatenate([Kg, yy[:, None]], axis=1))
    V, z = VV[:, :F], VV[:, F]
    return V.T @ z, qg - np.sum(V * V, axis=0), qg


def ulps(dev, ref):
    """the error of the two quantities in fp32 ulps of max(|ref|, 1e-3 S) (posterior_ref.ulp_error; S over the patient's functionals)"""
    return tuple(PR.ulp_error(d, r) for d, r in zip(dev[:2], ref[:2]))


def check_functional(ref, out):
    """One patient's device output (fmean[F], fvar[F]) against ref = restate(...): every element of both quantities within two fp32
    ulps of max(|ref|, 1e-3 S), S = the patient's largest |ref| of that quantity (the project's bar, posterior_ref.assert_fp32_close),
    and fvar <= q_g (1 + 2^-22): a posterior variance, never above the prior's.  Returns the two errors in ulps."""
    F = ref[0].shape[0]
    for k in range(2):
        assert out[k].shape == (F,) and out[k].dtype == np.float32, (NAMES[k], out[k].shape, out[k].dtype)
    if F == 0:
        return (0.0,) * 2
    for k in range(2):
        PR.assert_fp32_close(out[k], np.asarray(ref[k], np.float64), NAMES[k])
    assert np.all(out[1].astype(np.float64) <= np.asarray(ref[2], np.float64) * (1.0 + 2.0 ** -22)), "variance above the prior's"
    return tuple(PR.ulp_error(out[k], np.asarray(ref[k], np.float64)) for k in range(2))
