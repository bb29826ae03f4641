"""Rolling-origin forecasts of a patient's own observations and their scores (pure numpy; the predictions themselves come
from Context.forecast / medgp_forecast_batch).

rolling_origin() builds the points and prefixes of "what does the model predict at time t from what was known h hours
before t" (ref: main_one_test.cpp:269-300 builds such "past" sets one observation at a time).  score() restates the
quantities of the reference's evaluation (ref: medgpc/evaluation/evals.py:7-51: per feature, the mean absolute error and the
percentage of observations inside the 95 % interval) and adds the mean log predictive density.  training_prefix() builds the
history table of Context.forecast_grad / medgp_forecast_grad, which trains on that log predictive density.
"""
import numpy as np

CI95 = 1.96   # half-width of the 95 % interval in standard deviations


def rolling_origin(meta, t, y, horizons):
    """Forecast points of ONE patient whose observations are sorted by time (ValueError otherwise; ties are allowed).

    For every horizon h (hours, >= 0) in `horizons` and every observation i one point
        (meta_i, t_i, y_i, prefix = #{k : t_k < t_i - h}),
    horizon-major.  h = 0 is the strict one-step-ahead case: everything strictly earlier, so observations that share a time
    stamp (other covariates measured at the same moment) never condition on each other.  A horizon longer than the record
    gives prefix 0, the prior.  Uploaded in the same order, the patient's first `prefix` observations are exactly that set.
    Returns (meta2, t2, y2, prefix, hidx): int32 / float32 / float32 / int32 / int32 arrays of len(horizons) * n entries,
    hidx[j] = the index into `horizons` of point j.  meta = None (SE / SM) gives meta2 of zeros."""
    t = np.asarray(t, np.float32).ravel()
    y = np.asarray(y, np.float32).ravel()
    n = t.shape[0]
    m = np.zeros(n, np.int32) if meta is None else np.asarray(meta, np.int32).ravel()
    if y.shape[0] != n or m.shape[0] != n:
        raise ValueError(f"meta, t, y have {m.shape[0]}, {n}, {y.shape[0]} entries")
    if n > 1 and np.any(np.diff(t) < 0):
        raise ValueError("rolling_origin needs the observations sorted by time")
    hs = np.asarray(horizons, np.float64).ravel()
    if np.any(hs < 0) or not np.all(np.isfinite(hs)):
        raise ValueError("horizons must be finite and >= 0")
    t64 = t.astype(np.float64)
    # t sorted: the count of t_k < x is the left insertion point of x
    prefix = [np.searchsorted(t64, t64 - h, side="left") for h in hs]
    k = hs.shape[0]
    return (np.tile(m, k), np.tile(t, k), np.tile(y, k),
            (np.concatenate(prefix) if k else np.zeros(0)).astype(np.int32), np.repeat(np.arange(k, dtype=np.int32), n))


def training_prefix(t, horizon, min_history=0):
    """The prefix table of Context.forecast_grad / medgp_forecast_grad for ONE patient whose observations are sorted by time
    (ValueError otherwise; ties are allowed): per observation i the history length #{k : t_k < t_i - horizon}, i.e. rolling_origin's
    prefix for that horizon, and -1 (not scored) where that count is below min_history.  horizon in hours, >= 0; returns int32 [n]."""
    t = np.asarray(t, np.float32).ravel()
    if t.shape[0] > 1 and np.any(np.diff(t) < 0):
        raise ValueError("training_prefix needs the observations sorted by time")
    h = float(horizon)
    if not np.isfinite(h) or h < 0:
        raise ValueError("horizon must be finite and >= 0")
    if int(min_history) < 0:
        raise ValueError("min_history must be >= 0")
    t64 = t.astype(np.float64)
    p = np.searchsorted(t64, t64 - h, side="left").astype(np.int32)
    p[p < int(min_history)] = -1
    return p


def score(meta2, y2, hidx, mean, var, lpd=None, D=None, nh=None):
    """Per covariate d and horizon index h over the points with meta2 == d and hidx == h:
        mae[d, h]      mean |y2 - mean|,
        coverage[d, h] 100 x the share of points with |y2 - mean| <= 1.96 sqrt(var)   (per cent, as the reference reports it),
        lpd[d, h]      mean log predictive density (NaN everywhere when lpd is None),
        count[d, h]    the number of points.
    Points with a NaN prediction are left out (the reference's nanmean); a cell without points is NaN with count 0.
    Returns a dict of [D, nh] arrays."""
    meta2 = np.asarray(meta2, np.int64).ravel()
    hidx = np.asarray(hidx, np.int64).ravel()
    y2 = np.asarray(y2, np.float64).ravel()
    mean = np.asarray(mean, np.float64).ravel()
    var = np.asarray(var, np.float64).ravel()
    m = y2.shape[0]
    if not (meta2.shape[0] == hidx.shape[0] == mean.shape[0] == var.shape[0] == m):
        raise ValueError("meta2, y2, hidx, mean, var differ in length")
    ll = None if lpd is None else np.asarray(lpd, np.float64).ravel()
    if ll is not None and ll.shape[0] != m:
        raise ValueError("lpd differs in length")
    D = int(meta2.max()) + 1 if D is None and m else int(D or 0)
    nh = int(hidx.max()) + 1 if nh is None and m else int(nh or 0)
    out = {k: np.full((D, nh), np.nan) for k in ("mae", "coverage", "lpd")}
    out["count"] = np.zeros((D, nh), np.int64)
    err = np.abs(y2 - mean)
    with np.errstate(invalid="ignore"):
        inside = err <= CI95 * np.sqrt(var)
    valid = ~(np.isnan(mean) | np.isnan(var))
    for d in range(D):
        for h in range(nh):
            sel = valid & (meta2 == d) & (hidx == h)
            c = int(sel.sum())
            out["count"][d, h] = c
            if c == 0:
                continue
            out["mae"][d, h] = err[sel].mean()
            out["coverage"][d, h] = 100.0 * inside[sel].mean()
            if ll is not None:
                out["lpd"][d, h] = ll[sel].mean()
    return out
