"""The numpy side of the heteroscedastic calls (medgp_amd.robust), no GPU: the builders of scales and their range check, the
predictive interval of a Gaussian latent plus Student-t noise against its Gaussian limit, the constant of the bound, and the select_nu /
fit closures against a stand-in context that answers with robust.dense."""
import math

import numpy as np

import nlml_truth as T
from medgp_amd import robust


def test_helpers_build_scales():
    assert np.array_equal(robust.from_replicates([1, 2, 4]), [1.0, 0.5, 0.25])
    assert np.allclose(robust.from_sd([0.2, 0.4], 0.2), [1.0, 4.0])
    assert np.array_equal(robust.flagged([False, True], 50.0), [1.0, 50.0])
    for bad in (lambda: robust.from_replicates([0]), lambda: robust.flagged([True], np.inf), lambda: robust.from_sd([0.0], 1.0)):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("accepted")
    # the interval of a Gaussian latent plus t noise: wider than the Gaussian one of the same scale, symmetric, and at nu -> inf the Gaussian's
    lo, hi = robust.predictive_interval(1.0, 0.25, 0.09, 1e6, 0.95)
    assert abs((hi - lo) / 2 - 1.959964 * math.sqrt(0.34)) <= 2e-3 and abs((hi + lo) / 2 - 1.0) <= 1e-3
    lo3, hi3 = robust.predictive_interval(1.0, 0.25, 0.09, 3.0, 0.95)
    assert hi3 - lo3 > hi - lo and abs((hi3 + lo3) / 2 - 1.0) <= 1e-3
    assert abs(robust.kappa_const(1e9) + 5e8) <= 1e-3       # C(nu) -> -c as nu grows: kappa(nu, 1) -> 0


class _DenseCtx:
    """what fit and select_nu need of a Context, answered by robust.dense on an SE patient (no gradient: zeros)"""
    kernel_index, D, H = 0, 1, 3

    def __init__(self, t, y):
        self.t, self.y, self.calls = t, y, []

    def robust_nlml_grad(self, slots, theta, nu, sweeps=3, scale0=None, flag_grad=True, rows=True):
        theta = np.asarray(theta, np.float64).reshape(len(slots), 3)
        nu = np.broadcast_to(np.asarray(nu, np.float64).reshape(-1, 1) if np.size(nu) == len(slots) else np.asarray(nu, np.float64), (len(slots), 1))
        self.calls.append((len(slots), sweeps, None if scale0 is None else [a.copy() for a in scale0]))
        out = dict(obj=np.empty(len(slots)), grad=np.zeros((len(slots), 3)) if flag_grad else None, scale=[], delta=np.empty(len(slots)),
                   status=np.zeros(len(slots), np.int32), resid=None, fvar=None)
        for b in range(len(slots)):
            K = T.gram(0, 1, 1, 0, None, self.t, theta[b], np.float64, -1)
            r = robust.dense(K, self.y, math.exp(theta[b, 0]) ** 2, nu[b, 0], sweeps, None if scale0 is None else scale0[b])
            out["obj"][b], out["delta"][b] = r["obj"], r["delta"]
            out["scale"].append(r["scale"])
        return out


def _patient():
    g = T._philox(20262105, 0)
    t = np.sort(g.uniform(0.0, 50.0, size=40)).astype(np.float32)
    y = np.sin(t / 5.0) + 0.2 * g.standard_t(3.0, size=40)
    y[[3, 17, 30]] += 3.0          # three gross errors
    return t, y.astype(np.float64)


def test_select_nu_scans_the_grid_in_one_call():
    t, y = _patient()
    ctx = _DenseCtx(t, y)
    th = np.array([math.log(0.2), math.log(5.0), math.log(1.0)])
    J, best, st = robust.select_nu(ctx, 0, th, [1.0, 3.0, 10.0, 1e6], sweeps=10)
    assert len(ctx.calls) == 1 and ctx.calls[0][0] == 4 and J.shape == (4,) and np.all(st == 0)
    assert best == int(np.argmin(J)) and best != 3          # heavy-tailed noise: the Gaussian limit is not the best


def test_fit_warm_starts_the_scales():
    t, y = _patient()
    ctx = _DenseCtx(t, y)
    th = np.array([[math.log(0.2), math.log(5.0), math.log(1.0)]])
    fun, state = robust.fit(ctx, [0], th, 3.0, sweeps=2)
    j1, g1, _ = fun(th)
    j2, _, _ = fun(th)
    j3, _, _ = fun(th)
    assert ctx.calls[0][2] is None and ctx.calls[1][2] is not None
    four = robust.dense(T.gram(0, 1, 1, 0, None, t, th[0], np.float64, -1), y, math.exp(th[0, 0]) ** 2, 3.0, 4)["scale"]
    assert np.allclose(ctx.calls[2][2][0], four, rtol=1e-12, atol=0)     # the third evaluation starts where four sweeps end
    assert j1[0] >= j2[0] >= j3[0] and state["evals"] == 3 and g1.shape == (1, 3)   # the same theta: the sweeps go on where they stopped
