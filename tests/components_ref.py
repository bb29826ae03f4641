"""numpy definition of medgp_components_batch: the posterior of every spectral component f_q of the latent f = sum_q f_q at the test
points.  The reference program has no such output, so this file IS the definition (include/medgp_hip.h).

Component q is k_q(tau) = cos(w_q tau) exp(-c_q tau^2) with w_q, c_q and B_q as k_prep leaves them (trend_ref.hypers: SE is Q = 1 with
w = 0, SM has B_q = the 1 x 1 weight).  For a test point j = (m*, t*) and a training observation i = (m_i, t_i), tau = t* - t_i:
    K*_q[i]     = B_q[m_i, m*] k_q(tau)                       (sum_q K*_q = K* of posterior_ref)
    V_q = L^-1 K*_q,  z = L^-1 y,   L L^T = K + (1 + jitter_rounds) diag(sigma^2)
    cmean[j, q]   = V_q^T z
    ccov[j, q, r] = delta_qr B_q[m*, m*] - V_q^T V_r          (latent: no sigma^2)
    cvar[j, q]    = ccov[j, q, q].
restate() writes this down twice: in fp64 on numpy's LAPACK, and (dtype=np.longdouble) with its own Cholesky and forward solves, as
the truth the fp64 one is held to (test_components.py).  check_components() is the bound the GPU tests hold the device outputs to."""
import numpy as np

from oracle import oracle as O
import posterior_ref as PR
import trend_ref as TR

NAMES = ("cmean", "cvar", "ccov")


def restate(kidx, Q, D, R, meta, t, y, theta, meta2, t2, jitter_rounds=0, dtype=np.float64):
    """Returns (cmean[m, Q], cvar[m, Q], ccov[m, Q, Q], prior[m, Q]) in dtype; prior[j, q] = B_q[m*, m*].  meta / meta2 are ignored
    for SE / SM (may be None).  jitter_rounds = k: every quantity is that of the factor of K + k diag(sigma^2) that k retries leave."""
    sig2, B, w, c, meta, t, Lc = TR._train(kidx, Q, D, R, meta, t, theta, jitter_rounds, dtype)
    t2 = np.asarray(t2, np.float32).astype(dtype)
    yy = np.asarray(y, np.float32).astype(dtype)
    n, m = t.shape[0], t2.shape[0]
    meta2 = np.asarray(meta2, np.int64) if kidx == O.KERNEL_LMC_SM else np.zeros(m, np.int64)
    Kq = [TR._gram(B[q:q + 1], w[q:q + 1], c[q:q + 1], meta, t, meta2, t2) for q in range(Q)]     # Q x [n, m]
    VV = TR._solve(Lc, np.concatenate(Kq + [yy[:, None]], axis=1))
    V, z = VV[:, :Q * m].reshape(n, Q, m), VV[:, Q * m]
    cmean = np.einsum("iqj,i->jq", V, z)
    prior = np.stack([B[q][meta2, meta2] for q in range(Q)], axis=1).astype(dtype).reshape(m, Q)
    ccov = -np.einsum("iqj,irj->jqr", V, V)
    ccov[:, np.arange(Q), np.arange(Q)] += prior
    cvar = ccov[:, np.arange(Q), np.arange(Q)].copy()
    return cmean, cvar, ccov, prior


def ulps(dev, ref):
    """the error of each of the three quantities in fp32 ulps of max(|ref|, 1e-3 S) (posterior_ref.ulp_error; S over the whole array)"""
    return tuple(PR.ulp_error(d, r) for d, r in zip(dev[:3], ref[:3]))


def check_components(Q, ref, out):
    """One patient's device output (cmean[m, Q], cvar[m, Q], ccov[m, Q, Q] or None) against ref = restate(...): every element of
    every quantity within two fp32 ulps of max(|ref|, 1e-3 S), S = the patient's largest |ref| of that quantity (for ccov over the
    whole m x Q x Q block; the project's bar, posterior_ref.assert_fp32_close), and
        0 <= cvar <= B_q[m*, m*] (1 + 2^-22)                                a variance, never above the prior's
        ccov has exactly equal triangles, its diagonal has the bits of cvar
        |ccov_qr| <= sqrt(cvar_q cvar_r) (1 + 1e-5) + 2^-22 1e-3 S           Cauchy-Schwarz plus the bar's own floor
    Returns the three errors in ulps (ccov: 0.0 when None)."""
    m = ref[0].shape[0]
    shapes = ((m, Q), (m, Q), (m, Q, Q))
    for k in range(3):
        if out[k] is None:
            assert k == 2
            continue
        assert out[k].shape == shapes[k] and out[k].dtype == np.float32, (NAMES[k], out[k].shape, out[k].dtype)
    if m == 0:
        return (0.0,) * 3
    for k in range(3):
        if out[k] is not None:
            PR.assert_fp32_close(out[k], np.asarray(ref[k], np.float64), NAMES[k])
    cvar = out[1].astype(np.float64)
    prior = np.asarray(ref[3], np.float64)
    assert np.all(cvar >= 0.0), "negative component variance"
    assert np.all(cvar <= prior * (1.0 + 2.0 ** -22)), "component variance above the prior's"
    if out[2] is not None:
        cc = out[2]
        assert np.array_equal(cc.view(np.uint32), np.ascontiguousarray(cc.transpose(0, 2, 1)).view(np.uint32)), "ccov is not symmetric"
        dg = np.ascontiguousarray(cc[:, np.arange(Q), np.arange(Q)])
        assert np.array_equal(dg.view(np.uint32), np.ascontiguousarray(out[1]).view(np.uint32)), "diag(ccov) is not cvar"
        S = float(np.abs(np.asarray(ref[2], np.float64)).max())
        lim = np.sqrt(cvar[:, :, None] * cvar[:, None, :]) * (1.0 + 1e-5) + 2.0 ** -22 * 1e-3 * S
        assert np.all(np.abs(cc.astype(np.float64)) <= lim), "ccov beyond Cauchy-Schwarz"
    return tuple(PR.ulp_error(out[k], np.asarray(ref[k], np.float64)) if out[k] is not None else 0.0 for k in range(3))
