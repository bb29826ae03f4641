"""What the component posterior of Context.components / medgp_components_batch says about a patient (pure numpy; the posterior
itself comes from the device): which spectral component is which (its period, the length scale of its envelope, its weight on
every covariate), which components make up a band of periods, and the posterior of the sum of a band.

The prior is a sum of Q independent latent components, f = sum_q f_q, with k_q(tau) = cos(2 pi mu_q tau) exp(-2 (pi v_q tau)^2)
(include/medgp_hip.h).  Given the data the components of a point are jointly Gaussian with mean cmean[j] and covariance ccov[j], so
the sum over a band S is Gaussian with
    mean = sum_{q in S} cmean[j, q],      var = sum_{q, r in S} ccov[j, q, r]      (latent: no noise term).
"""
import math

import numpy as np

KERNEL_SE, KERNEL_LMC_SM, KERNEL_SM = 0, 7, 8


def table(kidx, Q, D, R, theta):
    """The components of a hyper-parameter vector in the theta layout of include/medgp_hip.h, as a dict of
        period_h [Q]    1 / mu_q, the period of the component in hours (inf for SE, which does not oscillate)
        length_h [Q]    1 / (2 pi v_q), the length scale of its envelope exp(-tau^2 / (2 length^2)) (SE: l)
        weight [Q, D']  B_q[d, d], the prior variance the component gives covariate d (D' = 1 for SE / SM: sf^2, the SM weight)"""
    th = np.asarray(theta, np.float64).ravel()
    if kidx == KERNEL_LMC_SM:
        if th.shape[0] != Q * (D * R + 2 + D) + D:
            raise ValueError(f"theta has {th.shape[0]} values, expected {Q * (D * R + 2 + D) + D}")
        A = th[D:D + Q * D * R].reshape(Q, D, R)
        o = D + Q * D * R
        mu, v = np.exp(th[o:o + Q]), np.exp(th[o + Q:o + 2 * Q])
        weight = np.sum(A * A, axis=2) + np.exp(th[o + 2 * Q:].reshape(Q, D))
    elif kidx == KERNEL_SM:
        if th.shape[0] != 1 + 3 * Q:
            raise ValueError(f"theta has {th.shape[0]} values, expected {1 + 3 * Q}")
        weight = np.exp(th[1:1 + Q]).reshape(Q, 1)
        mu, v = np.exp(th[1 + Q:1 + 2 * Q]), np.exp(th[1 + 2 * Q:1 + 3 * Q])
    elif kidx == KERNEL_SE:
        if Q != 1 or th.shape[0] != 3:
            raise ValueError(f"SE has Q = 1 and 3 hyper-parameters (Q = {Q}, {th.shape[0]} values)")
        return {"period_h": np.array([np.inf]), "length_h": np.exp(th[1:2]), "weight": np.exp(2.0 * th[2:3]).reshape(1, 1)}
    else:
        raise ValueError(f"kernel index {kidx}")
    return {"period_h": 1.0 / mu, "length_h": 1.0 / (2.0 * math.pi * v), "weight": weight}


def select(table, period_min=None, period_max=None):
    """Boolean mask [Q] of the components whose period lies in [period_min, period_max] hours (None: unbounded on that side; a
    component without a period -- SE -- counts as infinitely slow)."""
    p = np.asarray(table["period_h"], np.float64)
    mask = np.ones(p.shape, bool)
    if period_min is not None:
        mask &= p >= period_min
    if period_max is not None:
        mask &= p <= period_max
    return mask


def band(cmean, ccov, mask):
    """(mean [m], var [m]) of sum_{q in mask} f_q at every point, from cmean [m, Q] and ccov [m, Q, Q] of Context.components (summed in
    fp64).  An empty mask gives zeros; NaN inputs (a failed patient) give NaN."""
    cm = np.asarray(cmean, np.float64)
    cc = np.asarray(ccov, np.float64)
    mask = np.asarray(mask, bool)
    if cm.ndim != 2 or cc.shape != cm.shape + cm.shape[1:] or mask.shape != cm.shape[1:]:
        raise ValueError(f"cmean {cm.shape}, ccov {cc.shape}, mask {mask.shape}: expected [m, Q], [m, Q, Q], [Q]")
    return cm[:, mask].sum(axis=1), cc[:, mask][:, :, mask].sum(axis=(1, 2))
