"""Group tables for Context.loo and Context.lgo_grad: the usual ways to partition a patient's observations into held-out groups.
Pure numpy.  Every builder returns (group, ngroups): group[i] in [-1, ngroups) for observation i in the order the patient was
uploaded, -1 = never held out.  A patient's table goes into the `groups` list of Context.loo / Context.lgo_grad as it is."""
import numpy as np


def _ids(x):
    return np.ascontiguousarray(x, dtype=np.int32)


def by_covariate(meta, D=None):
    """leave-one-covariate-out: group = the observation's covariate; ngroups = D (default: largest covariate + 1)"""
    m = np.asarray(meta, dtype=np.int64).ravel()
    if m.size and m.min() < 0:
        raise ValueError("negative covariate index")
    G = int(m.max()) + 1 if m.size else 0
    if D is not None:
        if D < G:
            raise ValueError(f"covariate {G - 1} with D = {D}")
        G = int(D)
    return _ids(m), G


def _window(t, hours):
    t = np.asarray(t, dtype=np.float64).ravel()
    if not hours > 0:
        raise ValueError(f"window of {hours} hours")
    if t.size == 0:
        return np.zeros(0, np.int64), 0
    w = np.floor((t - t.min()) / float(hours)).astype(np.int64)
    return w, int(w.max()) + 1


def by_window(t, hours):
    """consecutive windows of the stay: group = floor((t - min t) / hours); windows without an observation are empty groups"""
    w, G = _window(t, hours)
    return _ids(w), G


def by_covariate_window(meta, t, hours, D=None):
    """one covariate missing for one window (the lab that was not drawn): group = window * D + covariate"""
    m, Dm = by_covariate(meta, D)
    w, G = _window(t, hours)
    if m.shape[0] != w.shape[0]:
        raise ValueError(f"{m.shape[0]} covariates for {w.shape[0]} times")
    if G * max(Dm, 1) > np.iinfo(np.int32).max:
        raise ValueError("too many groups")
    return _ids(w * Dm + m.astype(np.int64)), G * Dm


def k_fold(n, k, seed=0):
    """k random folds of n observations, sizes equal to +-1, the same table for the same (n, k, seed)"""
    if k < 1 or n < 0:
        raise ValueError(f"k_fold({n}, {k})")
    g = np.empty(n, np.int64)
    g[np.random.Generator(np.random.Philox(key=[int(seed), 0x6B666F6C64])).permutation(n)] = np.arange(n) % k
    return _ids(g), int(k)


def hold_out(n, idx):
    """one group holding the observations idx; everything else -1 (always conditioned on)"""
    idx = np.asarray(idx, dtype=np.int64).ravel()
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        raise ValueError("index outside [0, n)")
    g = np.full(n, -1, np.int64)
    g[idx] = 0
    return _ids(g), 1
