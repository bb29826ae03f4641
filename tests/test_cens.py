"""medgp_amd.censoring on numpy alone: the limits and flags of a lab feed become (y, code); the dense EP agrees with the definition
(cens_truth.py) and, for one censored row, with the closed form; impute returns the truncated normal whose moments are imp_mean and
imp_var; naive_bias shows the pull onto the limit and the shrunken variance.  No GPU."""
import math

import numpy as np
import pytest

import cens_truth as CT
import nlml_truth as T
import posterior_jvp_truth as PJ
from medgp_amd import censoring as cz


def test_from_limits_clips_and_codes():
    y = np.array([0.005, 0.2, 25.0, 3.0, 0.01, 1.0])
    m = np.array([0, 0, 1, 1, 0, 2])
    yy, code = cz.from_limits(y, lower=[0.01, np.nan, np.nan], upper=[np.nan, 20.0, np.nan], meta=m)
    assert list(code) == [-1, 0, 1, 0, -1, 0] and code.dtype == np.int8
    assert list(yy) == [0.01, 0.2, 20.0, 3.0, 0.01, 1.0]
    yy, code = cz.from_limits([0.5, 2.0, 9.0], lower=1.0, upper=8.0)
    assert list(code) == [-1, 0, 1] and list(yy) == [1.0, 2.0, 8.0]
    yy, code = cz.from_limits([0.5, 2.0])
    assert not np.any(code) and list(yy) == [0.5, 2.0]
    with pytest.raises(ValueError):
        cz.from_limits([1.0], lower=2.0, upper=0.5)


def test_codes_from_flags():
    assert list(cz.codes_from_flags(["<", "", ">", None, "<=", ">=", "=", " < "])) == [-1, 0, 1, 0, -1, 1, 0, -1]
    with pytest.raises(ValueError):
        cz.codes_from_flags(["~"])


def test_tail_is_accurate_far_below_zero():
    for z in (-35.0, -30.0, -8.0, -1.0, 0.0, 0.7, 3.0, 9.0):
        lz, r = cz.log_cdf_and_ratio(z)
        tl, tr = CT.tail(z, np.longdouble)
        assert abs(lz - float(tl)) <= 1e-14 * max(abs(float(tl)), 1e-300) and abs(r - float(tr)) <= 1e-14 * float(tr), z
    assert math.isfinite(cz.log_cdf_and_ratio(-1e4)[0]) and cz.log_cdf_and_ratio(40.0) == (0.0, 0.0)


def _dense(cid, p):
    c = CT.case(cid)
    m, t, y = c["pts"][p]
    K = T.gram(*CT.fam(c), m, t, c["th"][p], np.float64)
    return c, K, np.asarray(y, np.float64), c["code"][p]


def test_ep_dense_meets_the_definition():
    for cid, p in (("se", 2), ("sm_Q3", 1), ("lmc_D3_Q5", 1)):
        c, K, y, code = _dense(cid, p)
        r = cz.ep_dense(K, y, code)
        tr = CT.truth_of(c, p)
        n = int(np.sum(code != 0))
        e = CT.errors(dict(site=r["site"], imp_mean=r["imp_mean"], imp_var=r["imp_var"]), tr)
        assert n == tr["site"].shape[0] and r["sweeps"] == CT.programs_of(c, p)["b"]["sweeps"]
        assert max(e.values()) <= 1e-10, e


def test_exact_single_is_what_ep_gives_for_one_row():
    for cid, p in (("se", 0), ("sm_Q3", 0), ("lmc_D24", 0)):
        c, K, y, code = _dense(cid, p)
        tr = CT.objective(*CT.fam(c), *c["pts"][p], c["th"][p], code, np.longdouble)
        # (the definition carries the reference's PI in its log(2 pi) term)
        shift = (y.shape[0] - 1) * (math.log(2 * math.pi) - math.log(2 * T.REF_PI)) / 2
        assert abs(cz.exact_single(K, y, code) - shift - float(tr["nlml"])) <= 1e-10 * abs(float(tr["nlml_mag"])), (cid, p)
    with pytest.raises(ValueError):
        cz.exact_single(np.eye(3), np.zeros(3), [0, 0, 0])


def test_impute_returns_the_truncated_normal_behind_the_ep_moments():
    c, K, y, code = _dense("sm_Q3", 4)
    r = cz.ep_dense(K, y, code)
    idx = r["idx"]
    out = cz.impute(y[idx], code[idx], r["imp_mean"], r["imp_var"], r["site"], probs=(0.05, 0.5, 0.95))
    # at the fixed point the truncated cavity has the moments EP reports
    assert np.allclose(out["mean"], r["imp_mean"], rtol=0, atol=1e-9) and np.allclose(out["var"], r["imp_var"], rtol=1e-8)
    below = code[idx] == cz.BELOW
    assert np.all(out["mean"][below] < y[idx][below]) and np.all(out["mean"][~below] > y[idx][~below])
    q = out["quant"]
    assert np.all(np.diff(q, axis=1) > 0) and np.all(q[below] <= y[idx][below, None]) and np.all(q[~below] >= y[idx][~below, None])
    # the caller's units: value = center + scale * z-score
    o2 = cz.impute(y[idx], code[idx], r["imp_mean"], r["imp_var"], r["site"], center=2.0, scale=3.0, probs=(0.5,))
    assert np.allclose(o2["mean"], 2.0 + 3.0 * out["mean"]) and np.allclose(o2["var"], 9.0 * out["var"]) and np.allclose(o2["sd"], 3.0 * out["sd"])
    assert np.allclose(o2["quant"][:, 0], 2.0 + 3.0 * q[:, 1])
    # a Monte-Carlo look at one row: the truncated normal N(loc, sd^2) beyond the limit
    g = np.random.default_rng(5)
    k = 0
    draws = out["loc"][k] + out["sd"][k] * g.standard_normal(400000)
    keep = draws <= y[idx][k] if code[idx][k] == cz.BELOW else draws >= y[idx][k]
    assert abs(draws[keep].mean() - out["mean"][k]) <= 5 * out["sd"][k] / math.sqrt(keep.sum()) + 1e-3


def test_naive_bias_shows_the_pull_onto_the_limit():
    c, K, y, code = _dense("sm_Q3", 1)
    m, t, _ = c["pts"][1]
    idx = np.where(code != 0)[0]
    t2 = t[idx].copy()                                        # the points: the censored rows' own time stamps
    Ks, kss, s2 = PJ.cross_gram(*CT.fam(c), m, t, c["th"][1], None, t2, np.float64)
    nb = cz.naive_bias(K, y, code, Ks, kss + s2)
    post = CT.posterior(*CT.fam(c), m, t, y, c["th"][1], code, None, t2, np.float64)
    assert np.allclose(nb["mean_cens"], post["mean"], atol=1e-8) and np.allclose(nb["var_cens"], post["var"], rtol=1e-8)
    assert np.all(nb["var_ratio"] < 1.0)                       # a limit taken as an observation claims knowledge it does not have
    # BELOW rows: the value lies below the limit, so the naive mean (pulled onto the limit) is too high there
    k = int(np.argmax(nb["shift"]))                            # the strongly binding row of the "far7" placement
    assert code[idx[k]] == cz.BELOW and nb["shift"][k] > 0.5
