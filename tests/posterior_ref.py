"""numpy restatement of GP_Regression::parsed_predict (ref: core/gp_regression.cpp:216-320) on top of the oracle's Gram
matrix: posterior mean and variance at the test points, and the part of the mean carried by the training observations of
each covariate,
    part_d[j] = mean_func[j] + sum_{k: meta[k] == d} K*[k, j] alpha[k],   alpha = K^-1 y   (zero mean function here).
K, K* and k** + sigma^2 come from ONE oracle Gram matrix of the training points followed by the test points (the noise
only sits on the diagonal, so the off-diagonal block is the cross Gram of c_kernel_*::compute_cross_gram_matrix)."""
import numpy as np

from oracle import oracle as O


def restate(kidx, Q, D, R, meta, t, y, theta, meta2, t2):
    """Returns (mean[m], var[m], parts[m, D]) in fp64 (D = 1 for SE / SM)."""
    t = np.asarray(t, np.float32)
    t2 = np.asarray(t2, np.float32)
    n, m = t.shape[0], t2.shape[0]
    multi = kidx == O.KERNEL_LMC_SM
    Dp = D if multi else 1
    meta = np.asarray(meta, np.int32) if multi else np.zeros(n, np.int32)
    meta2 = np.asarray(meta2, np.int32) if multi else np.zeros(m, np.int32)
    K = O.gram(kidx, Q, D, R, np.concatenate([meta, meta2]) if multi else None, np.concatenate([t, t2]), theta)
    Kxx, Ks, kss = K[:n, :n], K[:n, n:], np.diag(K[n:, n:])
    Lc = np.linalg.cholesky(Kxx)
    yy = np.asarray(y, np.float32).astype(np.float64)
    alpha = np.linalg.solve(Lc.T, np.linalg.solve(Lc, yy))
    V = np.linalg.solve(Lc, Ks)
    mean = Ks.T @ alpha
    var = kss - np.sum(V * V, axis=0)
    parts = np.zeros((m, Dp))
    for d in range(Dp):
        sel = meta == d
        parts[:, d] = Ks[sel].T @ alpha[sel]
    return mean, var, parts
