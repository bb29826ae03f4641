"""numpy restatement of GP_Regression::parsed_predict (ref: core/gp_regression.cpp:216-320) on top of the oracle's Gram
matrix: posterior mean and variance at the test points, and the part of the mean carried by the training observations of
each covariate,
    part_d[j] = mean_func[j] + sum_{k: meta[k] == d} K*[k, j] alpha[k],   alpha = K^-1 y   (zero mean function here).
K, K* and k** + sigma^2 come from ONE oracle Gram matrix of the training points followed by the test points (the noise
only sits on the diagonal, so the off-diagonal block is the cross Gram of c_kernel_*::compute_cross_gram_matrix).

check_posterior() is the bound the GPU tests hold the device outputs to (fp32 outputs of an fp64 computation)."""
import numpy as np

from oracle import oracle as O

# |dev - ref| <= FP32_BOUND * max(|ref|, FLOOR * S): two fp32 ulps of the larger of |ref| and a floor relative to the largest
# |ref| of that quantity in the patient (S).  A correct kernel is off by the fp32 rounding of an fp64 result (<= 2^-24
# relative) plus fp64 error scaled by cond(K) ~ 1e2 of the synthetic patients, i.e. well inside the bound.
FP32_BOUND = 2.0 ** -22
FLOOR = 1e-3


def noise_var(kidx, D, theta, meta2):
    """sigma^2 of the test points' covariates (the likelihood hypers theta[:D] are log sigma; one for SE / SM)"""
    sig2 = np.exp(2.0 * np.asarray(theta, np.float64)[:D if kidx == O.KERNEL_LMC_SM else 1])
    return sig2[np.asarray(meta2, np.int64)] if kidx == O.KERNEL_LMC_SM else np.full(len(meta2), sig2[0])


def terms(kidx, Q, D, R, meta, t, y, theta, meta2, t2, jitter_rounds=0):
    """(K*, alpha, L, k**, sigma^2_{meta2}, meta) of the restatement; meta is all zeros for SE / SM.  The factor is of
    K + jitter_rounds * diag(sigma^2_{meta}): what the reference's retry loop factors after that many extra noise additions
    (ref: c_inference_exact.cpp:99-111)."""
    t = np.asarray(t, np.float32)
    t2 = np.asarray(t2, np.float32)
    n, m = t.shape[0], t2.shape[0]
    multi = kidx == O.KERNEL_LMC_SM
    meta = np.asarray(meta, np.int32) if multi else np.zeros(n, np.int32)
    meta2 = np.asarray(meta2, np.int32) if multi else np.zeros(m, np.int32)
    K = O.gram(kidx, Q, D, R, np.concatenate([meta, meta2]) if multi else None, np.concatenate([t, t2]), theta)
    Kxx, Ks, kss = K[:n, :n].copy(), K[:n, n:], np.diag(K[n:, n:]).copy()
    sig2_2 = noise_var(kidx, D, theta, meta2)
    kss -= sig2_2                                   # k** without the noise (the Gram diagonal carries it once)
    if jitter_rounds:
        Kxx[np.diag_indices(n)] += jitter_rounds * noise_var(kidx, D, theta, meta)
    Lc = np.linalg.cholesky(Kxx)
    yy = np.asarray(y, np.float32).astype(np.float64)
    alpha = np.linalg.solve(Lc.T, np.linalg.solve(Lc, yy))
    return Ks, alpha, Lc, kss, sig2_2, meta


def restate(kidx, Q, D, R, meta, t, y, theta, meta2, t2, jitter_rounds=0):
    """Returns (mean[m], var[m], parts[m, D]) in fp64 (D = 1 for SE / SM).  jitter_rounds = k: the posterior of the factor
    of K + k diag(sigma^2) that k retries leave; the noise of the test points is still added once,
    var = k** - q + sigma^2_{meta2} (oracle/medgp_oracle.c, medgp_oracle_fit_predict)."""
    Ks, alpha, Lc, kss, sig2_2, meta = terms(kidx, Q, D, R, meta, t, y, theta, meta2, t2, jitter_rounds)
    Dp = D if kidx == O.KERNEL_LMC_SM else 1
    V = np.linalg.solve(Lc, Ks)
    mean = Ks.T @ alpha
    var = kss - np.sum(V * V, axis=0) + sig2_2
    parts = np.zeros((Ks.shape[1], Dp))
    for d in range(Dp):
        sel = meta == d
        parts[:, d] = Ks[sel].T @ alpha[sel]
    return mean, var, parts


def ulp_error(dev, ref):
    """max |dev - ref| / (2^-23 max(|ref|, FLOOR * S)): the error in fp32 ulps of the larger of |ref| and the floor"""
    ref = np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    scale = np.maximum(np.abs(ref), FLOOR * np.abs(ref).max())
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(np.asarray(dev, np.float64) - ref) / (2.0 ** -23 * scale)
    return float(np.nanmax(np.where(np.isnan(e), np.inf, e)))


def assert_fp32_close(dev, ref, what):
    dev = np.asarray(dev, np.float64)
    ref = np.asarray(ref, np.float64)
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    if ref.size == 0:
        return
    scale = np.maximum(np.abs(ref), FLOOR * np.abs(ref).max())
    bad = ~(np.abs(dev - ref) <= FP32_BOUND * scale)   # (NaN fails)
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, np.abs(dev - ref) / scale, -1.0))), ref.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.size} elements beyond 2 fp32 ulps; worst at {i}: dev {dev[i]!r} "
                             f"ref {ref[i]!r} ({ulp_error(dev, ref):.2f} ulps)")


def check_posterior(kidx, D, theta, meta2, ref, mean, var, parts=None):
    """The device's (mean, var, parts) of one patient against ref = restate(...) (or its parts).  Every element within two fp32
    ulps of max(|ref|, 1e-3 S), S = the patient's max |ref| of that quantity; the parts of a point sum to its mean; the latent
    posterior variance is >= 0 (var >= sigma^2_{meta2} up to the fp32 rounding of the sum)."""
    rm, rv, rp = ref
    m = rm.shape[0]
    assert mean.shape == (m,) and var.shape == (m,)
    if m == 0:
        return
    assert_fp32_close(mean, rm, "mean")
    assert_fp32_close(var, rv, "var")
    sig2 = noise_var(kidx, D, theta, meta2 if kidx == O.KERNEL_LMC_SM else np.zeros(m, np.int32))
    # fp64 slack 1e-12 k**, with the patient's largest reference var standing in for k** (a point far from the data has
    # var = k** + sigma^2)
    assert np.all(var.astype(np.float64) >= sig2 * (1.0 - 2.0 ** -23) - 1e-12 * np.abs(rv).max()), "var below the noise"
    if parts is not None:
        assert parts.shape == rp.shape, (parts.shape, rp.shape)
        assert_fp32_close(parts, rp, "parts")
        Dp = rp.shape[1]
        ps = np.abs(rp).max()
        # the parts of a point sum to its mean, to float rounding
        assert np.all(np.abs(parts.astype(np.float64).sum(axis=1) - mean) <= 4e-7 * (Dp + 1) * (ps + np.abs(mean)))
