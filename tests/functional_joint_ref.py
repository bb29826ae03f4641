"""numpy definition of medgp_functional_joint_batch: the joint posterior of a patient's linear functionals g_f = sum_{k in f} a_k
f_{m_k}(t_k) of the latent function.  The reference program has no such output, so this file IS the definition (include/medgp_hip.h).

With the T terms of all F functionals of the patient side by side, A the [T, F] weight matrix (column f holds the weights of f's terms,
zero elsewhere) and K_tt the prior covariance of the latent function at the terms (component q: k_q(tau) = cos(w_q tau) exp(-c_q tau^2),
hypers as k_prep leaves them, trend_ref.hypers):
    K*_g  = K_nt A                                  [n, F]
    V     = L^-1 K*_g,  z = L^-1 y,                 L L^T = K + (1 + jitter_rounds) diag(sigma^2)
    fmean = V^T z
    Q     = A^T K_tt A                              the prior covariance of the functionals
    fcov  = Q - V^T V                               LATENT: no sigma^2 anywhere
    fvar  = diag(fcov)
restate() writes this down twice: in fp64 on numpy's LAPACK, and (dtype=np.longdouble) with trend_ref's own Cholesky and forward
solves, as the truth the fp64 one is held to (test_functional_joint.py).  check_joint() is the bound the GPU tests hold the device
outputs to."""
import functools

import numpy as np

from oracle import oracle as O
import posterior_ref as PR
import trend_ref as TR

NAMES = ("fmean", "fvar", "fcov")


def restate(kidx, Q, D, R, meta, t, y, theta, toffsets, meta2, t2, weight, jitter_rounds=0, dtype=np.float64):
    """Returns (fmean[F], fvar[F], fcov[F, F], Q_prior[F, F]) in dtype for the F = len(toffsets) - 1 functionals whose terms are
    [toffsets[f], toffsets[f + 1]) of meta2 / t2 / weight.  meta / meta2 are ignored for SE / SM (may be None).  jitter_rounds = k:
    every quantity is that of the factor of K + k diag(sigma^2) that k retries leave."""
    sig2, B, w, c, meta, t, Lc = TR._train(kidx, Q, D, R, meta, t, theta, jitter_rounds, dtype)
    toff = np.asarray(toffsets, np.int64)
    t2 = np.asarray(t2, np.float32).astype(dtype)
    a = np.asarray(weight, np.float64).astype(dtype)
    yy = np.asarray(y, np.float32).astype(dtype)
    T, F = t2.shape[0], toff.shape[0] - 1
    assert toff[0] == 0 and toff[-1] == T == a.shape[0]
    meta2 = np.asarray(meta2, np.int64) if kidx == O.KERNEL_LMC_SM else np.zeros(T, np.int64)
    A = np.zeros((T, F), dtype)
    for f in range(F):
        A[int(toff[f]):int(toff[f + 1]), f] = a[int(toff[f]):int(toff[f + 1])]
    Kg = TR._gram(B, w, c, meta, t, meta2, t2) @ A                              # [n, F]
    Qp = A.T @ (TR._gram(B, w, c, meta2, t2, meta2, t2) @ A)
    Qp = (Qp + Qp.T) / 2
    VV = TR._solve(Lc, np.concatenate([Kg, yy[:, None]], axis=1))
    V, z = VV[:, :F], VV[:, F]
    fcov = Qp - V.T @ V
    fcov = (fcov + fcov.T) / 2
    return V.T @ z, np.diag(fcov).copy(), fcov, Qp


def ulps(dev, ref):
    """the error of the three quantities in fp32 ulps of max(|ref|, 1e-3 S) (posterior_ref.ulp_error; S over the patient's functionals,
    for fcov over its whole F x F block)"""
    return tuple(PR.ulp_error(d, r) for d, r in zip(dev[:3], ref[:3]))


def check_joint(ref, out):
    """One patient's device output (fmean[F], fvar[F], fcov[F, F]) against ref = restate(...): every element of the three quantities
    within two fp32 ulps of max(|ref|, 1e-3 S), S = the patient's largest |ref| of that quantity (the project's bar,
    posterior_ref.assert_fp32_close; for fcov over the whole block); fcov exactly symmetric; its diagonal the bits of fvar.  Returns
    the three errors in ulps."""
    F = ref[0].shape[0]
    for k, shape in enumerate(((F,), (F,), (F, F))):
        assert out[k].shape == shape and out[k].dtype == np.float32, (NAMES[k], out[k].shape, out[k].dtype)
    if F == 0:
        return (0.0,) * 3
    for k in range(3):
        PR.assert_fp32_close(out[k], np.asarray(ref[k], np.float64), NAMES[k])
    bits = np.ascontiguousarray(out[2]).view(np.uint32)
    assert np.array_equal(bits, bits.T), "fcov is not exactly symmetric"
    assert np.array_equal(np.diag(bits), np.ascontiguousarray(out[1]).view(np.uint32)), "the diagonal of fcov does not have the bits of fvar"
    return tuple(PR.ulp_error(out[k], np.asarray(ref[k], np.float64)) for k in range(3))


def restate_case(fam, pt, th, packed, jitter_rounds=0, dtype=np.float64):
    """restate() on a patient of functional_cases (fam = (kernel, Q, D, R), pt = (meta, t, y), packed as functionals.pack returns it)"""
    import functional_cases as FC
    toff, m2, t2, a = packed
    return restate(*FC.fam_args(fam, pt), th, toff, m2 if fam[0] == O.KERNEL_LMC_SM else None, t2, a, jitter_rounds, dtype)


@functools.lru_cache(maxsize=None)
def case_ref(name, p, dtype=np.float64):
    """restate() of patient p of functional_cases.CASES[name] (computed once per process, shared by the tests; treat as read-only)"""
    import functional_cases as FC
    fam, pts, th, qs = FC.case_data(name)
    return restate_case(fam, pts[p], th[p], qs[p], FC.JITTER_ROUNDS.get(name, 0), dtype)
