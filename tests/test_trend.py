"""medgp_trend_batch without a GPU: the ABI surface and the argument errors that need no device; the definition (trend_ref.py)
held against posterior_ref for the order-0 terms and against finite differences of the long-double posterior for the slope terms;
the fp64 restatement against the long-double one on every input of the GPU tests (trend_cases.py), which is the condition under
which the GPU tests' bar measures the device and not the reference; the far-field limit; Context.trend's argument checks and the
helpers of medgp_amd/trend.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import medgp_amd
from medgp_amd import capi, synth, trend
import forecast_ref as FR
import posterior_ref as PR
import trend_cases as TC
import trend_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 2.0 ** -6    # step of the finite differences; the points sit on a grid of H so that t +- H and t +- 2 H are exact in float


def test_header_declares_and_library_exports_trend(built_lib):
    src = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    assert re.search(r"int\s+medgp_trend_batch\s*\(", src)
    for ref in ("core/gp_regression.cpp:128-214", "kernel/c_kernel_LMC_SM.cpp:329-372", "tests/trend_ref.py", "2^14"):
        assert ref in src, ref
    assert hasattr(C.CDLL(built_lib), "medgp_trend_batch")
    assert "medgp_trend_batch" in capi.SYMBOLS
    lib = capi.load()
    assert lib.medgp_abi_version() >= 9
    names = [lib.medgp_profile_kernel_name(k).decode() for k in range(lib.medgp_profile_num_kernels())]
    # k_trend sits in front of k_forecast, which test_forecast.py requires to stay the last name: ids 0 .. 20 did not move, and
    # every caller in the tree addresses a kernel by its name (Context.profile_enable(only=...), profile_read)
    assert names.count("k_trend") == 1 and names[21] == "k_trend" and names[-1] == "k_forecast" and len(names) == 23
    assert names[11] == "k_posterior" and names[18:21] == ["k_loo_kinv", "k_loo_vec", "k_loo_wgrad"]
    assert b"k_trend" in open(built_lib, "rb").read()


def test_null_context_and_null_outputs_are_argument_errors(built_lib):
    """The argument checks run before any device work; without a context (and so without a device) every call is MEDGP_ERR_ARG."""
    lib = capi.load()
    i32, i64, f32, f64 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))), \
        (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    slots, th, off = np.zeros(1, np.int32), np.zeros(8), np.array([0, 1], np.int64)
    m2, t2, st = np.zeros(1, np.int32), np.zeros(1, np.float32), np.zeros(1, np.int32)
    o = [np.zeros(1, np.float32) for _ in range(5)]
    full = [None, 1, i32(slots), f64(th), i64(off), i32(m2), f32(t2)] + [f32(a) for a in o] + [i32(st)]
    assert lib.medgp_trend_batch(*full) == -1   # MEDGP_ERR_ARG
    for drop in ((2,), (3,), (4,), (9,), (10,), (9, 10), (11,)):
        a = list(full)
        for k in drop:
            a[k] = None
        assert lib.medgp_trend_batch(*a) == -1, drop


def _grid_points(seed, D, t, m):
    """m points on the grid of H inside the patient's range, away from its ends"""
    g = np.random.default_rng(seed)
    lo, hi = math.ceil(float(t.min())) + 1, math.floor(float(t.max())) - 1
    t2 = (lo + np.floor(g.uniform(0, hi - lo, size=m) / H) * H).astype(np.float32)
    return g.integers(0, D, size=m).astype(np.int32), t2


SHAPES = [(7, 3, 3, 2, 131), (7, 5, 24, 8, 300), (7, 2, 2, 2, 200), (8, 3, 1, 0, 140), (0, 1, 1, 0, 90)]


@pytest.fixture(scope="module", params=SHAPES, ids=[f"k{s[0]}Q{s[1]}D{s[2]}n{s[4]}" for s in SHAPES])
def shape(request):
    """(family args with the patient, theta, meta2, t2, the long-double restatement at the points) of one shape"""
    kidx, Q, D, R, n = request.param
    pt = synth.patient(61, n, D, n, interleave=True)
    th = synth.theta(61, n, kidx, Q, D, R)
    m2, t2 = _grid_points(n, D, pt[1], 24)
    args = TC.fam_args((kidx, Q, D, R), pt)
    return args, th, m2, t2, TR.restate(*args, th, m2, t2, dtype=np.longdouble)


def test_order0_terms_match_posterior_ref(shape):
    """mean and var of trend_ref (its own Gram matrix, from oracle.coregional and the reference's PI) against posterior_ref.restate
    (the oracle's Gram matrix): 1e-12 of the largest |ref| of the quantity"""
    args, th, m2, t2, _ = shape
    a = TR.restate(*args, th, m2, t2)
    r = PR.restate(*args, th, m2 if args[0] == 7 else None, t2)
    for k in (0, 1):
        e = float(np.abs(a[k] - r[k]).max() / np.abs(r[k]).max())
        print(f"{TR.NAMES[k]}: {e:.3g}")
        assert e <= 1e-12


def _richardson(f):
    """4th-order central difference from steps H and 2 H: (4 D(H) - D(2 H)) / 3"""
    return (4.0 * f(H) - f(2.0 * H)) / 3.0


def _scale(args, th):
    """Lambda^2 = max_q (w_q^2 + 2 c_q): the largest -k_q''(0), the squared angular-frequency scale of the prior"""
    _, _, w, c = TR.hypers(*args[:4], th)
    return float(np.max(w * w + 2.0 * c))


def test_dmean_is_the_derivative_of_the_mean(shape):
    """dmean against the Richardson central difference of the long-double posterior mean: 1e-8 of the largest |dmean|"""
    args, th, m2, t2, ld = shape
    t2d = t2.astype(np.float64)

    def mean_at(s):
        return TR.restate(*args, th, m2, (t2d + s).astype(np.float32), dtype=np.longdouble)[0]
    fd = _richardson(lambda h: (mean_at(h) - mean_at(-h)) / (2.0 * h))
    e = float(np.abs(fd - ld[2]).max() / np.abs(ld[2]).max())
    print(f"dmean vs Richardson: {e:.3g}")
    assert e <= 1e-8


def test_dvar_and_cross_are_derivatives_of_the_covariance(shape):
    """With C(a, b) the posterior covariance of the latent f: var (f(t + h) - f(t - h)) / 2h = dvar + O(h^2) and
    cov(f(t), (f(t + h) - f(t - h)) / 2h) = cross + O(h^2); Richardson removes the h^2 term.  The tolerance, relative to the prior
    scale Lambda^2 k(0) of dvar (Lambda k(0) of cross), Lambda^2 = max_q -k_q''(0), has two terms derived from h:
      truncation  the h^4 term carries a sixth derivative of the covariance, of order Lambda^6 k(0): (Lambda H)^4, times 4 for the
                  Richardson weights (4 + 16) / 3 and the Taylor coefficients;
      rounding    the second difference cancels four values of C, each known to eps cond(K) k(0) in long double (eps = 2^-63;
                  the solves lose at most cond(K)), over 4 H^2: eps cond(K) / (Lambda H)^2, times 2 for the Richardson weights
                  (4 + 1) / 3.  It is the larger term for a smooth kernel (SE with a long length scale)."""
    args, th, m2, t2, ld = shape
    t2d = t2.astype(np.float64)
    lam2 = _scale(args, th)
    cond = FR.cond(*args[:6], th)
    tol = 4.0 * (lam2 * H * H) ** 2 + 2.0 * float(np.finfo(np.longdouble).eps) * cond / (lam2 * H * H)
    f32 = lambda x: x.astype(np.float32)

    def cov(sa, sb):
        return TR.latent_cov(*args[:6], th, m2, f32(t2d + sa), m2, f32(t2d + sb))
    fd_var = _richardson(lambda h: (cov(h, h) - 2.0 * cov(h, -h) + cov(-h, -h)) / (4.0 * h * h))
    fd_cross = _richardson(lambda h: (cov(0.0, h) - cov(0.0, -h)) / (2.0 * h))
    prior_var = float(np.max(ld[5])) / lam2 if lam2 > 0 else 0.0     # >= k(0) of the covariates (k''** <= Lambda^2 k**)
    ev = float(np.abs(fd_var - ld[3]).max() / np.max(ld[5]))
    ec = float(np.abs(fd_cross - ld[4]).max() / math.sqrt(float(np.max(ld[5])) * prior_var))
    print(f"(Lambda H)^4 = {(lam2 * H * H) ** 2:.3g}, cond {cond:.3g}, tolerance {tol:.3g}; dvar vs Richardson: {ev:.3g}; cross vs Richardson: {ec:.3g}")
    assert ev <= tol and ec <= tol
    # and the slope's variance is a real reduction of the prior's
    assert np.all(ld[3] > 0) and np.all(ld[3] < ld[5])


@pytest.mark.parametrize("name", list(TC.CASES))
def test_fp64_restatement_is_far_inside_the_bar(name):
    """On every input of the GPU tests the fp64 restatement and the long-double one differ by at most 0.01 x the bar of 2 fp32
    ulps of max(|ref|, 1e-3 S), in all five outputs: the bar then measures the device, not the reference."""
    fam, pts, th, qs = TC.case_data(name)
    worst = [0.0] * 5
    for p in TC.checked(name):
        if qs[p][1].shape[0] == 0:
            continue
        a, b = TC.case_ref(name, p), TC.case_ref(name, p, np.longdouble)
        u = TR.ulps(a, [np.asarray(x, np.float64) for x in b])
        worst = [max(x, y) for x, y in zip(worst, u)]
        assert np.all(a[3] >= 0) and np.all(a[3] <= a[5])
    print(name, " ".join(f"{n} {x:.2g}" for n, x in zip(TR.NAMES, worst)), "(fp32 ulps)")
    assert max(worst) <= 0.01 * 2.0


def test_far_field_limit():
    """|t* - t| >= 5000 h: every envelope exp(-c_q tau^2) has underflowed, the data say nothing about the slope there"""
    fam, pt, th, (m2, t2), prior = TC.far_case()
    assert min(float(t2[:fam[2]].min()) - float(pt[1].max()), float(pt[1].min()) - float(t2[fam[2]:].max())) >= 5000.0 - 1.0
    for dtype in (np.float64, np.longdouble):   # (long double does not underflow there, but nothing is left in a float)
        mean, var, dmean, dvar, cross, pr = TR.restate(*TC.fam_args(fam, pt), th, m2, t2, dtype=dtype)
        for x in (mean, dmean, cross):
            assert np.all(np.abs(x) < 2.0 ** -150) and np.all(x.astype(np.float32) == 0.0)
        if dtype == np.float64:
            assert np.all(dmean == 0.0) and np.all(cross == 0.0) and np.array_equal(dvar, pr)
        assert np.array_equal(dvar.astype(np.float32), pr.astype(np.float32))
        assert np.allclose(np.asarray(pr, np.float64), prior, rtol=1e-15)


# ---- Context.trend and medgp_amd/trend.py ----------------------------------------------------------------------------------

class _Lib:
    def medgp_trend_batch(self, *a):
        raise AssertionError("the library must not be reached")


def _bare_context(kidx, D, Hn):
    ctx = object.__new__(medgp_amd.Context)    # no device: the checks under test run before the library is called
    ctx._lib, ctx._h, ctx.kernel_index, ctx.D, ctx.H = _Lib(), None, kidx, D, Hn
    return ctx


def test_context_trend_argument_validation():
    ctx = _bare_context(7, 3, 10)
    th = np.zeros((2, 10))
    t2 = [np.zeros(3, np.float32), np.zeros(0, np.float32)]
    m2 = [np.zeros(3, np.int32), np.zeros(0, np.int32)]
    with pytest.raises(ValueError, match="theta has"):
        ctx.trend([0, 1], np.zeros((2, 9)), m2, t2)
    with pytest.raises(ValueError, match="test-point arrays"):
        ctx.trend([0, 1], th, m2, t2[:1])
    with pytest.raises(ValueError, match="required for the multi-output"):
        ctx.trend([0, 1], th, None, t2)
    with pytest.raises(ValueError, match="covariate arrays"):
        ctx.trend([0, 1], th, m2[:1], t2)
    with pytest.raises(ValueError, match="covariates for"):
        ctx.trend([0, 1], th, [m2[0][:2], m2[1]], t2)
    with pytest.raises(AssertionError, match="must not be reached"):   # a well-formed call does go on to the library
        ctx.trend([0, 1], th, m2, t2)
    assert hasattr(medgp_amd, "prob_rising") and hasattr(medgp_amd, "rate_interval") and hasattr(medgp_amd, "grid")
    assert medgp_amd.trend is trend


def test_prob_rising():
    dm = np.array([0.0, 1.0, -1.0, 1.96, 3.0, -3.0, 0.5])
    dv = np.array([1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.25])
    p = trend.prob_rising(dm, dv)
    assert p.dtype == np.float64 and p.shape == dm.shape
    exp = [0.5, 0.8413447460685429, 0.15865525393145707, 0.9750021048517795, 1.0, 0.0, 0.8413447460685429]
    np.testing.assert_allclose(p, exp, rtol=1e-14, atol=0)
    assert trend.prob_rising(0.0, 0.0) == 0.5
    assert 0.0 < trend.prob_rising(-30.0, 1.0) < 1e-190    # the lower tail does not cancel to zero
    assert np.all(np.isnan(trend.prob_rising(np.array([np.nan, 1.0, 1.0]), np.array([1.0, np.nan, -1.0]))))
    assert trend.prob_rising(np.float32(2.0), np.float32(4.0)) == pytest.approx(0.8413447460685429, rel=1e-14)
    with pytest.raises(ValueError):
        trend.prob_rising(np.zeros(2), np.zeros(3))


def test_rate_interval():
    lo, hi = trend.rate_interval(np.array([1.0, -2.0]), np.array([4.0, 0.0]))
    np.testing.assert_allclose(lo, [1.0 - 2 * 1.959963984540054, -2.0], rtol=1e-14)
    np.testing.assert_allclose(hi, [1.0 + 2 * 1.959963984540054, -2.0], rtol=1e-14)
    lo, hi = trend.rate_interval(0.0, 1.0, level=0.5)
    assert hi == pytest.approx(0.6744897501960817, rel=1e-12) and lo == -hi
    assert np.isnan(trend.rate_interval(np.nan, 1.0)[0]) and np.isnan(trend.rate_interval(1.0, -1.0)[1])
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            trend.rate_interval(0.0, 1.0, level=bad)


def test_grid():
    m2, t2 = trend.grid([3.0, 10.0, 5.5], 2, 2.0)
    assert m2.dtype == np.int32 and t2.dtype == np.float32
    assert np.array_equal(t2, [3, 5, 7, 9, 10, 3, 5, 7, 9, 10]) and np.array_equal(m2, [0] * 5 + [1] * 5)
    m2, t2 = trend.grid([0.0, 6.0], 1, 2.0)                # the last step lands on t_max: it is not repeated
    assert np.array_equal(t2, [0, 2, 4, 6]) and np.array_equal(m2, [0] * 4)
    m2, t2 = trend.grid([7.0], 3, 1.0)                     # one observation: one time per covariate
    assert np.array_equal(t2, [7, 7, 7]) and np.array_equal(m2, [0, 1, 2])
    m2, t2 = trend.grid([], 3, 1.0)
    assert m2.shape == t2.shape == (0,)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            trend.grid([0.0, 1.0], 1, bad)
    with pytest.raises(ValueError):
        trend.grid([0.0, 1.0], 0, 1.0)
    with pytest.raises(ValueError):
        trend.grid([0.0, float("nan")], 1, 1.0)
