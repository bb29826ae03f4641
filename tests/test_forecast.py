"""medgp_forecast_batch without a GPU: the ABI surface, the argument errors that need no device, the one-factor identity
against the refit definition on every input of the GPU tests (forecast_cases.py) together with the condition their error bars
rest on, and rolling_origin / score on hand-made patients."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from medgp_amd import capi, forecast
import forecast_cases as FC
import forecast_ref as FR
import posterior_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COND_MAX = 1e6


def test_header_declares_and_library_exports_forecast(built_lib):
    src = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    assert re.search(r"int\s+medgp_forecast_batch\s*\(", src)
    for ref in ("core/gp_regression.cpp:128-214", "main_one_test.cpp:269-300", "medgpc/evaluation/evals.py:7-51"):
        assert ref in src, ref
    assert hasattr(C.CDLL(built_lib), "medgp_forecast_batch")
    assert "medgp_forecast_batch" in capi.SYMBOLS
    lib = capi.load()
    assert lib.medgp_abi_version() >= 8
    names = [lib.medgp_profile_kernel_name(k).decode() for k in range(lib.medgp_profile_num_kernels())]
    # appended: the ids of the earlier kernels did not move
    assert names[-1] == "k_forecast" and names[18:21] == ["k_loo_kinv", "k_loo_vec", "k_loo_wgrad"]
    assert b"k_forecast" in open(built_lib, "rb").read()


def test_null_context_is_an_argument_error(built_lib):
    """The argument checks run before any device work; without a context (and so without a device) every call is
    MEDGP_ERR_ARG, whatever else is wrong with it."""
    lib = capi.load()
    i32, i64, f32, f64 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))), \
        (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    slots, th, off = np.zeros(1, np.int32), np.zeros(8), np.array([0, 1], np.int64)
    m2, t2, pf, y2 = np.zeros(1, np.int32), np.zeros(1, np.float32), np.zeros(1, np.int32), np.zeros(1, np.float32)
    mean, var, lpd, st = np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1), np.zeros(1, np.int32)
    full = [None, 1, i32(slots), f64(th), i64(off), i32(m2), f32(t2), i32(pf), f32(y2), f32(mean), f32(var), f64(lpd), i32(st)]
    assert lib.medgp_forecast_batch(*full) == -1   # MEDGP_ERR_ARG
    for drop in ((2,), (3,), (4,), (7,), (8,), (11,), (8, 11), (6, 9, 10), (12,)):
        a = list(full)
        for k in drop:
            a[k] = None
        assert lib.medgp_forecast_batch(*a) == -1, drop
    a = list(full)
    a[1] = 0
    assert lib.medgp_forecast_batch(*a) == -1


@pytest.fixture(scope="module")
def spread():
    return {"lpd": 0.0, "cases": 0}


@pytest.mark.parametrize("i", range(len(FC.CASES)), ids=[FC.case_id(s) for s in FC.CASES])
def test_one_factor_identity_equals_the_refit(i, spread):
    """rows < p of solve(L, K*) against a refit of obs[0:p], for every patient of the case: mean / var at 1/8 of the device's
    bar (two fp64 programs), and cond(K) <= 1e6 -- a condition on the INPUTS under which that bar can be asked of fp64 work."""
    fam, pts, th, qs = FC.case_data(i)
    for p, pt in enumerate(pts):
        assert FR.cond(*FC.fam_args(fam, pt)[:6], th[p]) <= COND_MAX, (i, p)
        m2, t2, y2, pf = qs[p]
        ref = FC.case_ref(i, p)
        one = FR.one_factor(*FC.fam_args(fam, pt), th[p], m2 if fam[0] == 7 else None, t2, pf, y2)
        if t2.shape[0] == 0:
            continue
        for k in (0, 1):
            if np.any(ref[k] != 0):
                assert PR.ulp_error(one[k], ref[k]) <= 0.25, (i, p, k)
            else:
                assert np.all(one[k] == 0)
        assert np.all(one[0][pf == 0] == 0.0)
        e = FR.lpd_error(one[2], ref[2])
        print(f"case {i} patient {p}: n {pt[1].shape[0]} m {t2.shape[0]} lpd spread {e:.3g}")
        spread["lpd"] = max(spread["lpd"], e)
    spread["cases"] += 1


def test_lpd_spread_is_recorded(spread):
    """The largest |one-factor - refit| of lpd over the cases, relative to max(1, |ref|), is what the GPU test's bound is built
    from (forecast_ref.lpd_bound).  tests/golden/forecast_lpd_spread.json holds the figure recorded with the cases' seed
    (MEDGP_RECORD_GOLDEN=1 rewrites it); any other run must see the same cases and stay inside the bound derived from it --
    two fp64 programs may differ between numpy builds, by the summation-order factor the bound allows the device."""
    assert spread["cases"] == len(FC.CASES), "run the whole module: the spread is taken over every case"
    if os.environ.get("MEDGP_RECORD_GOLDEN") == "1":
        json.dump({"seed": FC.SEED, "cases": [FC.case_id(s) for s in FC.CASES], "lpd_spread": spread["lpd"],
                   "what": "max |one_factor - refit| of lpd / max(1, |refit|) over tests/forecast_cases.py (fp64, numpy)"},
                  open(FR.GOLDEN, "w"), indent=1)
    rec = json.load(open(FR.GOLDEN))
    assert rec["seed"] == FC.SEED and rec["cases"] == [FC.case_id(s) for s in FC.CASES]
    assert 0.0 < rec["lpd_spread"] < 1e-10
    assert spread["lpd"] <= FR.lpd_bound(), (spread["lpd"], rec["lpd_spread"])


def test_identity_under_jitter():
    fam, pts, th, qs = FC.case_data(0)
    m2, t2, y2, pf = qs[0]
    one = FR.one_factor(*FC.fam_args(fam, pts[0]), th[0], m2, t2, pf, y2, jitter_rounds=2)
    ref = FC.case_ref(0, 0, 2)
    assert PR.ulp_error(one[0], ref[0]) <= 0.25 and PR.ulp_error(one[1], ref[1]) <= 0.25
    assert FR.lpd_error(one[2], ref[2]) <= FR.lpd_bound()


# ---- rolling_origin / score ------------------------------------------------------------------------------------------------

def test_rolling_origin_prefixes():
    # three covariates measured together at t = 0 and t = 10, one alone at t = 4 and t = 30
    meta = np.array([0, 1, 2, 1, 0, 1, 2, 2], np.int32)
    t = np.array([0, 0, 0, 4, 10, 10, 10, 30], np.float32)
    y = np.arange(8, dtype=np.float32)
    m2, t2, y2, pf, hi = forecast.rolling_origin(meta, t, y, [0, 6, 100])
    assert m2.dtype == np.int32 and t2.dtype == np.float32 and y2.dtype == np.float32 and pf.dtype == np.int32 and hi.dtype == np.int32
    assert np.array_equal(m2, np.tile(meta, 3)) and np.array_equal(t2, np.tile(t, 3)) and np.array_equal(y2, np.tile(y, 3))
    assert np.array_equal(hi, np.repeat([0, 1, 2], 8))
    # h = 0: strictly earlier -- tied time stamps never condition on each other
    assert np.array_equal(pf[:8], [0, 0, 0, 3, 4, 4, 4, 7])
    # h = 6: t_k < t_i - 6  (t = 10: the three at 0, not the one at 4 = 10 - 6; t = 30: all seven before)
    assert np.array_equal(pf[8:16], [0, 0, 0, 0, 3, 3, 3, 7])
    # a horizon longer than the record: the prior everywhere
    assert np.array_equal(pf[16:], np.zeros(8, np.int32))
    # brute force
    for j in range(24):
        assert pf[j] == int(np.sum(t.astype(np.float64) < float(t2[j]) - [0, 6, 100][hi[j]]))


def test_rolling_origin_rejects_bad_input():
    with pytest.raises(ValueError, match="sorted by time"):
        forecast.rolling_origin([0, 0, 0], [0.0, 2.0, 1.0], [1.0, 2.0, 3.0], [0])
    with pytest.raises(ValueError):
        forecast.rolling_origin([0, 0], [0.0, 1.0], [1.0], [0])
    with pytest.raises(ValueError):
        forecast.rolling_origin([0, 0], [0.0, 1.0], [1.0, 2.0], [-1.0])
    m2, t2, y2, pf, hi = forecast.rolling_origin(None, [0.0, 1.0], [1.0, 2.0], [])
    assert m2.shape == t2.shape == y2.shape == pf.shape == hi.shape == (0,)
    m2, _, _, pf, _ = forecast.rolling_origin(None, [0.0, 1.0], [1.0, 2.0], [0])
    assert np.array_equal(m2, [0, 0]) and np.array_equal(pf, [0, 1])


def test_score_by_hand():
    meta2 = np.array([0, 0, 1, 1, 0, 0])
    hidx = np.array([0, 0, 0, 0, 1, 1])
    y2 = np.array([1.0, 2.0, 0.0, 0.0, 1.0, 5.0])
    mean = np.array([0.0, 2.5, 1.0, np.nan, 1.0, 1.0])
    var = np.array([1.0, 0.01, 0.25, 1.0, 4.0, 4.0])
    lpd = np.array([-1.0, -2.0, -3.0, -4.0, -5.0, -7.0])
    s = forecast.score(meta2, y2, hidx, mean, var, lpd)
    assert s["mae"].shape == (2, 2)
    # d = 0, h = 0: errors 1 (inside 1.96) and 0.5 (outside 0.196)
    assert s["mae"][0, 0] == 0.75 and s["coverage"][0, 0] == 50.0 and s["lpd"][0, 0] == -1.5 and s["count"][0, 0] == 2
    # d = 1, h = 0: the NaN prediction is left out; error 1 > 1.96 * 0.5
    assert s["mae"][1, 0] == 1.0 and s["coverage"][1, 0] == 0.0 and s["lpd"][1, 0] == -3.0 and s["count"][1, 0] == 1
    # d = 0, h = 1: errors 0 and 4 against 3.92
    assert s["mae"][0, 1] == 2.0 and s["coverage"][0, 1] == 50.0 and s["lpd"][0, 1] == -6.0
    # d = 1, h = 1: no point
    assert np.isnan(s["mae"][1, 1]) and np.isnan(s["coverage"][1, 1]) and s["count"][1, 1] == 0
    s2 = forecast.score(meta2, y2, hidx, mean, var, None, D=3, nh=2)
    assert s2["mae"].shape == (3, 2) and np.all(np.isnan(s2["lpd"])) and np.array_equal(s2["mae"][:2], s["mae"], equal_nan=True)
    with pytest.raises(ValueError):
        forecast.score(meta2, y2[:3], hidx, mean, var)
