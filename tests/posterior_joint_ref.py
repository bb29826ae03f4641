"""numpy restatement of the joint posterior of a patient's test points (medgp_posterior_joint_batch), on top of ONE oracle
Gram matrix of the training points followed by the test points, as posterior_ref.terms:
    C  = K** - V^T V + diag(sigma^2_{meta2}),   V = L^-1 K*      (the Gram diagonal carries the test points' noise once)
    Lc = chol(C) (lower, in the caller's order of the points),   samples = mean + Lc eps
The reference has no such function: this IS the definition.  diag(C) is posterior_ref.restate's var.

check_joint() holds device output to the project's bar (posterior_ref.FP32_BOUND = 2 fp32 ulps of max(|ref|, 1e-3 S)).  That
bar needs C well conditioned: an fp64 factorisation moves the samples by about cond(C) 2^-53, far under 2^-24 only while
cond(C) is moderate.  This is a condition on the INPUTS, asserted here for every case: cond(C) <= COND_MAX."""
import numpy as np

from oracle import oracle as O
from posterior_ref import assert_fp32_close, noise_var

COND_MAX = 1e4


def restate_joint(kidx, Q, D, R, meta, t, y, theta, meta2, t2, jitter_rounds=0):
    """Returns (mean[m], var[m], C[m, m], Lc[m, m]) in fp64.  jitter_rounds = k: the factor of K + k diag(sigma^2) that k
    retries leave; the noise of the test points is still added once."""
    t = np.asarray(t, np.float32)
    t2 = np.asarray(t2, np.float32)
    n, m = t.shape[0], t2.shape[0]
    multi = kidx == O.KERNEL_LMC_SM
    meta = np.asarray(meta, np.int32) if multi else np.zeros(n, np.int32)
    meta2 = np.asarray(meta2, np.int32) if multi else np.zeros(m, np.int32)
    K = O.gram(kidx, Q, D, R, np.concatenate([meta, meta2]) if multi else None, np.concatenate([t, t2]), theta)
    Kxx, Ks, Kss = K[:n, :n].copy(), K[:n, n:], K[n:, n:]
    if jitter_rounds:
        Kxx[np.diag_indices(n)] += jitter_rounds * noise_var(kidx, D, theta, meta)
    L = np.linalg.cholesky(Kxx)
    V = np.linalg.solve(L, Ks)
    z = np.linalg.solve(L, np.asarray(y, np.float32).astype(np.float64))
    mean = V.T @ z
    C = Kss - V.T @ V
    C = 0.5 * (C + C.T)
    Lc = np.linalg.cholesky(C) if m else np.zeros((0, 0))
    return mean, np.diag(C).copy(), C, Lc


def draw(ref, eps):
    """samples[m, nsamp] = mean + Lc eps of ref = restate_joint(...)"""
    mean, _, _, Lc = ref
    return mean[:, None] + Lc @ np.asarray(eps, np.float64)


def cond(C):
    w = np.linalg.eigvalsh(C)
    return float(w[-1] / w[0])


def check_joint(ref, var, cov=None, samples=None, eps=None):
    """One patient's device output against ref = restate_joint(...): cov within the bar of C (S = the largest |C_ij|), exactly
    symmetric, its diagonal within the bar of the device's var; samples within the bar of mean + Lc eps (S = the patient's
    largest |sample|).  The inputs must be well conditioned (module docstring)."""
    mean, rvar, C, Lc = ref
    m = mean.shape[0]
    if m == 0:
        assert cov is None or cov.shape == (0, 0)
        assert samples is None or samples.shape[0] == 0
        return
    assert cond(C) <= COND_MAX, f"test input: cond(C) = {cond(C):.3g}"
    if cov is not None:
        assert cov.shape == (m, m) and cov.dtype == np.float32
        assert np.array_equal(cov.view(np.uint32), cov.T.view(np.uint32)), "cov is not bitwise symmetric"
        assert_fp32_close(cov, C, "cov")
        # the diagonal against the marginal output, same bar (floor: the patient's largest |C_ij|)
        S = np.abs(C).max()
        dv = np.asarray(var, np.float64)
        assert np.all(np.abs(np.diag(cov).astype(np.float64) - dv) <= 2.0 ** -22 * np.maximum(np.abs(dv), 1e-3 * S)), "diag(cov) != var"
    if samples is not None:
        rs = draw(ref, eps)
        assert samples.shape == rs.shape and samples.dtype == np.float32
        assert_fp32_close(samples, rs, "samples")
