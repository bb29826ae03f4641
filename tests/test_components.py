"""medgp_components_batch without a GPU: the ABI surface and the argument errors that need no device; the definition
(components_ref.py) held against posterior_ref (the components of a point sum to its posterior) and its covariance blocks checked for
symmetry and positive semi-definiteness; the fp64 restatement against the long-double one on every input of the GPU tests
(components_cases.py), which is the condition under which the GPU tests' bar measures the device and not the reference; the far-field
limit; Context.components' argument checks and the helpers of medgp_amd/components.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import medgp_amd
from medgp_amd import capi, components, synth
import components_cases as CC
import components_ref as CR
import posterior_ref as PR
import trend_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_components(built_lib):
    src = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    assert re.search(r"int\s+medgp_components_batch\s*\(", src)
    for ref in ("core/gp_regression.cpp:128-214", "kernel/c_kernel_LMC_SM.cpp:329-372", "tests/components_ref.py", "2^14", "2 fp32 ulps"):
        assert ref in src[src.index("Posterior of every spectral COMPONENT"):src.index("int medgp_components_batch")], ref
    assert hasattr(C.CDLL(built_lib), "medgp_components_batch")
    assert "medgp_components_batch" in capi.SYMBOLS
    lib = capi.load()
    assert lib.medgp_abi_version() >= 10
    # the kernel has no profile entry of its own (its launches are accounted under k_posterior), but it is in the library
    names = [lib.medgp_profile_kernel_name(k).decode() for k in range(lib.medgp_profile_num_kernels())]
    assert "k_components" not in names and names[11] == "k_posterior"
    assert b"k_components" in open(built_lib, "rb").read()


def test_null_context_and_null_outputs_are_argument_errors(built_lib):
    """The argument checks run before any device work; without a context (and so without a device) every call is MEDGP_ERR_ARG."""
    lib = capi.load()
    i32, i64, f32, f64 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))), \
        (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    slots, th, off = np.zeros(1, np.int32), np.zeros(8), np.array([0, 1], np.int64)
    m2, t2, st = np.zeros(1, np.int32), np.zeros(1, np.float32), np.zeros(1, np.int32)
    o = [np.zeros(4, np.float32) for _ in range(3)]
    full = [None, 1, i32(slots), f64(th), i64(off), i32(m2), f32(t2)] + [f32(a) for a in o] + [i32(st)]
    assert lib.medgp_components_batch(*full) == -1   # MEDGP_ERR_ARG
    for drop in ((2,), (3,), (4,), (7,), (8,), (7, 8), (9,)):
        a = list(full)
        for k in drop:
            a[k] = None
        assert lib.medgp_components_batch(*a) == -1, drop


# ---- the definition -----------------------------------------------------------------------------------------------------------

SHAPES = [(7, 3, 3, 2, 131), (7, 5, 24, 8, 300), (7, 2, 2, 2, 200), (7, 17, 2, 1, 90), (8, 3, 1, 0, 140), (0, 1, 1, 0, 90)]


@pytest.fixture(scope="module", params=SHAPES, ids=[f"k{s[0]}Q{s[1]}D{s[2]}n{s[4]}" for s in SHAPES])
def shape(request):
    """(family args with the patient, theta, meta2, t2, the fp64 restatement at the points) of one shape"""
    kidx, Q, D, R, n = request.param
    pt = synth.patient(62, n, D, n, interleave=True)
    th = synth.theta(62, n, kidx, Q, D, R)
    m2, t2 = CC.points(n, D, pt[1], 24)
    args = CC.fam_args((kidx, Q, D, R), pt)
    return args, th, m2, t2, CR.restate(*args, th, m2, t2)


def test_components_sum_to_the_posterior(shape):
    """sum_q cmean = mean and sum_qr ccov + sigma^2 = var of posterior_ref.restate (the oracle's Gram matrix): 1e-12 of the largest
    |ref| of the quantity"""
    args, th, m2, t2, (cmean, cvar, ccov, prior) = shape
    rm, rv, _ = PR.restate(*args, th, m2 if args[0] == 7 else None, t2)
    sig2 = PR.noise_var(args[0], args[2], th, m2 if args[0] == 7 else np.zeros(len(t2), np.int32))
    em = float(np.abs(cmean.sum(axis=1) - rm).max() / np.abs(rm).max())
    ev = float(np.abs(ccov.sum(axis=(1, 2)) + sig2 - rv).max() / np.abs(rv).max())
    print(f"mean: {em:.3g}  var: {ev:.3g}")
    assert em <= 1e-12 and ev <= 1e-12
    assert np.array_equal(cvar, ccov[:, np.arange(args[1]), np.arange(args[1])])


def test_component_covariance_is_symmetric_and_psd(shape):
    """ccov[j] is the posterior covariance of (f_1 .. f_Q) at the point: symmetric, smallest eigenvalue >= -1e-12 x trace, and a
    component's variance is a real reduction of its prior's"""
    args, th, m2, t2, (cmean, cvar, ccov, prior) = shape
    assert np.array_equal(ccov, ccov.transpose(0, 2, 1))
    for j in range(ccov.shape[0]):
        ev = np.linalg.eigvalsh(ccov[j])
        assert ev[0] >= -1e-12 * np.trace(ccov[j]), (j, ev[0], np.trace(ccov[j]))
    assert np.all(cvar > 0) and np.all(cvar <= prior)


@pytest.mark.parametrize("name", list(CC.CASES))
def test_fp64_restatement_is_far_inside_the_bar(name):
    """On every input of the GPU tests the fp64 restatement and the long-double one differ by at most 0.01 x the bar of 2 fp32
    ulps of max(|ref|, 1e-3 S), in cmean, cvar and ccov: the bar then measures the device, not the reference."""
    fam, pts, th, qs = CC.case_data(name)
    worst = [0.0] * 3
    for p in CC.checked(name):
        if qs[p][1].shape[0] == 0:
            continue
        a, b = CC.case_ref(name, p), CC.case_ref(name, p, np.longdouble)
        u = CR.ulps(a, [np.asarray(x, np.float64) for x in b])
        worst = [max(x, y) for x, y in zip(worst, u)]
        assert np.all(a[1] >= 0) and np.all(a[1] <= a[3]), "cvar outside [0, prior]"
    print(name, " ".join(f"{n} {x:.2g}" for n, x in zip(CR.NAMES, worst)), "(fp32 ulps)")
    assert max(worst) <= 0.01 * 2.0


def test_far_field_limit():
    """|t* - t| >= 5000 h: every envelope exp(-c_q tau^2) has underflowed, the data say nothing about any component there"""
    fam, pt, th, (m2, t2), prior = CC.far_case()
    Q = fam[1]
    assert min(float(t2[:fam[2]].min()) - float(pt[1].max()), float(pt[1].min()) - float(t2[fam[2]:].max())) >= 5000.0 - 1.0
    off = ~np.eye(Q, dtype=bool)
    for dtype in (np.float64, np.longdouble):   # (long double does not underflow there, but nothing is left in a float)
        cmean, cvar, ccov, pr = CR.restate(*CC.fam_args(fam, pt), th, m2, t2, dtype=dtype)
        for x in (cmean, ccov[:, off]):
            assert np.all(np.abs(x) < 2.0 ** -150) and np.all(x.astype(np.float32) == 0.0)
        if dtype == np.float64:
            assert np.all(cmean == 0.0) and np.all(ccov[:, off] == 0.0) and np.array_equal(cvar, pr)
        assert np.array_equal(cvar.astype(np.float32), pr.astype(np.float32))
        assert np.allclose(np.asarray(pr, np.float64), prior, rtol=1e-15)


# ---- Context.components and medgp_amd/components.py ----------------------------------------------------------------------------

class _Lib:
    def medgp_components_batch(self, *a):
        raise AssertionError("the library must not be reached")


def _bare_context(kidx, Q, D, Hn):
    ctx = object.__new__(medgp_amd.Context)    # no device: the checks under test run before the library is called
    ctx._lib, ctx._h, ctx.kernel_index, ctx.Q, ctx.D, ctx.H = _Lib(), None, kidx, Q, D, Hn
    return ctx


def test_context_components_argument_validation():
    ctx = _bare_context(7, 2, 3, 10)
    th = np.zeros((2, 10))
    t2 = [np.zeros(3, np.float32), np.zeros(0, np.float32)]
    m2 = [np.zeros(3, np.int32), np.zeros(0, np.int32)]
    with pytest.raises(ValueError, match="theta has"):
        ctx.components([0, 1], np.zeros((2, 9)), m2, t2)
    with pytest.raises(ValueError, match="test-point arrays"):
        ctx.components([0, 1], th, m2, t2[:1])
    with pytest.raises(ValueError, match="required for the multi-output"):
        ctx.components([0, 1], th, None, t2)
    with pytest.raises(ValueError, match="covariate arrays"):
        ctx.components([0, 1], th, m2[:1], t2)
    with pytest.raises(ValueError, match="covariates for"):
        ctx.components([0, 1], th, [m2[0][:2], m2[1]], t2)
    with pytest.raises(AssertionError, match="must not be reached"):   # a well-formed call does go on to the library
        ctx.components([0, 1], th, m2, t2)
    assert medgp_amd.components is components and "components" in medgp_amd.__all__


def test_table():
    # LMC-SM, Q = 2, D = 2, R = 1: [log sigma (2) | A (Q D R) | log mu (Q) | log v (Q) | log kappa (Q D)]
    th = np.array([0.1, 0.2, 1.0, -2.0, 0.5, 3.0, math.log(1 / 24.0), math.log(0.5), math.log(1 / (2 * math.pi * 10.0)), math.log(1 / (2 * math.pi)),
                   math.log(0.25), math.log(4.0), 0.0, math.log(2.0)])
    tb = components.table(7, 2, 2, 1, th)
    np.testing.assert_allclose(tb["period_h"], [24.0, 2.0], rtol=1e-14)
    np.testing.assert_allclose(tb["length_h"], [10.0, 1.0], rtol=1e-14)
    np.testing.assert_allclose(tb["weight"], [[1.0 + 0.25, 4.0 + 4.0], [0.25 + 1.0, 9.0 + 2.0]], rtol=1e-14)
    # ... and it is the diagonal of the B_q the definition uses
    _, B, w, c = TR.hypers(7, 2, 2, 1, th)
    np.testing.assert_allclose(tb["weight"], np.stack([np.diag(B[q]) for q in range(2)]), rtol=1e-13)
    # SM, Q = 2: [log sigma | log weight | log mu | log v]
    tb = components.table(8, 2, 1, 0, np.log([0.3, 2.0, 5.0, 0.125, 1.0, 1 / (2 * math.pi * 3.0), 0.5]))
    np.testing.assert_allclose(tb["period_h"], [8.0, 1.0], rtol=1e-14)
    np.testing.assert_allclose(tb["length_h"], [3.0, 1 / math.pi], rtol=1e-14)
    np.testing.assert_allclose(tb["weight"], [[2.0], [5.0]], rtol=1e-14)
    # SE: [log sigma | log l | log sf]
    tb = components.table(0, 1, 1, 0, np.log([0.3, 7.0, 3.0]))
    assert np.isinf(tb["period_h"][0]) and tb["length_h"][0] == pytest.approx(7.0, rel=1e-14) and tb["weight"][0, 0] == pytest.approx(9.0, rel=1e-14)
    for bad in ((7, 2, 2, 1, np.zeros(13)), (8, 2, 1, 0, np.zeros(6)), (0, 1, 1, 0, np.zeros(2)), (0, 2, 1, 0, np.zeros(3)), (3, 1, 1, 0, np.zeros(3))):
        with pytest.raises(ValueError):
            components.table(*bad)


def test_select():
    tb = {"period_h": np.array([24.0, 2.0, np.inf, 168.0])}
    assert np.array_equal(components.select(tb), [True] * 4)
    assert np.array_equal(components.select(tb, period_min=24.0), [True, False, True, True])
    assert np.array_equal(components.select(tb, period_max=24.0), [True, True, False, False])
    assert np.array_equal(components.select(tb, 12.0, 200.0), [True, False, False, True])
    assert components.select(tb, 300.0, 400.0).dtype == bool and not components.select(tb, 300.0, 400.0).any()


def test_band():
    cmean = np.array([[1.0, 2.0, 4.0], [0.5, -1.0, 0.25]], np.float32)
    ccov = np.array([[[1.0, 0.1, 0.2], [0.1, 2.0, 0.3], [0.2, 0.3, 3.0]], [[4.0, -1.0, 0.0], [-1.0, 5.0, 0.5], [0.0, 0.5, 6.0]]], np.float32)
    mean, var = components.band(cmean, ccov, [True, False, True])
    assert mean.dtype == np.float64 and var.dtype == np.float64
    np.testing.assert_allclose(mean, [5.0, 0.75], rtol=1e-7)
    np.testing.assert_allclose(var, [1.0 + 3.0 + 2 * 0.2, 4.0 + 6.0], rtol=1e-7)
    mean, var = components.band(cmean, ccov, [True, True, True])
    np.testing.assert_allclose(var, [6.0 + 2 * 0.6, 15.0 - 2.0 + 1.0], rtol=1e-7)
    mean, var = components.band(cmean, ccov, [False] * 3)
    assert np.all(mean == 0.0) and np.all(var == 0.0)
    assert np.all(np.isnan(components.band(np.full((1, 3), np.nan), np.full((1, 3, 3), np.nan), [True, False, False])[0]))
    for bad in ((cmean, ccov[:, :2], [True] * 3), (cmean, ccov, [True] * 2), (cmean[0], ccov[0], [True] * 3)):
        with pytest.raises(ValueError):
            components.band(*bad)
