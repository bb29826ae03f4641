"""medgp_functional_batch without a GPU: the ABI surface and the argument errors that need no device; the definition
(functional_ref.py) held against what exists -- a single term of weight 1 is posterior_ref's point, a general functional is
a^T (C - diag sigma^2) a and a^T mean of posterior_joint_ref -- with 0 <= fvar <= q_g and the far-field limit; the fp64 restatement
against the long-double one on every input of the GPU tests (functional_cases.py), which is the condition under which the GPU tests'
bar measures the device and not the reference; Context.functionals' argument checks and the builders of medgp_amd/functionals.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import medgp_amd
from medgp_amd import capi, functionals, synth
import functional_cases as FC
import functional_ref as FR
import posterior_joint_ref as PJ
import posterior_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_functional(built_lib):
    src = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    assert re.search(r"int\s+medgp_functional_batch\s*\(", src)
    doc = src[src.index("Posterior of LINEAR FUNCTIONALS"):src.index("int medgp_functional_batch")]
    for ref in ("core/gp_regression.cpp:128-214", "kernel/c_kernel_LMC_SM.cpp:329-372", "tests/functional_ref.py", "2^14", "2 fp32 ulps",
                "no clamp", "REORDERING", "slope terms", "covariance BETWEEN two", "observation noise"):
        assert ref in doc, ref
    assert hasattr(C.CDLL(built_lib), "medgp_functional_batch")
    assert "medgp_functional_batch" in capi.SYMBOLS
    lib = capi.load()
    assert lib.medgp_abi_version() >= 11
    # the kernels have no profile entry of their own (k_functional is accounted under k_posterior), but they are in the library
    names = [lib.medgp_profile_kernel_name(k).decode() for k in range(lib.medgp_profile_num_kernels())]
    assert len(names) == 23 and names[0] == "k_prep" and names[11] == "k_posterior" and names[21] == "k_trend" and names[22] == "k_forecast"
    assert not any("functional" in n for n in names)
    blob = open(built_lib, "rb").read()
    assert b"k_functional" in blob and b"k_functional_prep" in blob


def test_null_context_and_null_or_broken_arguments_are_argument_errors(built_lib):
    """The argument checks run before any device work; without a context (and so without a device) every call is MEDGP_ERR_ARG."""
    lib = capi.load()
    i32, i64, f32, f64 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))), \
        (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    slots, th, st = np.zeros(1, np.int32), np.zeros(8), np.zeros(1, np.int32)
    foff, toff = np.array([0, 2], np.int64), np.array([0, 1, 3], np.int64)
    m2, t2, a = np.zeros(3, np.int32), np.zeros(3, np.float32), np.ones(3)
    o = [np.full(2, 7.0, np.float32) for _ in range(2)]
    full = [None, 1, i32(slots), f64(th), i64(foff), i64(toff), i32(m2), f32(t2), f64(a), f32(o[0]), f32(o[1]), i32(st)]
    assert lib.medgp_functional_batch(*full) == -1   # MEDGP_ERR_ARG
    for drop in range(2, 12):
        args = list(full)
        args[drop] = None
        assert lib.medgp_functional_batch(*args) == -1, drop
    for bf, bt in (([1, 2], [0, 1, 3]), ([0, -1], [0, 1, 3]), ([0, 2], [1, 1, 3]), ([0, 2], [0, 3, 1])):
        args = list(full)
        args[4], args[5] = i64(np.array(bf, np.int64)), i64(np.array(bt, np.int64))
        assert lib.medgp_functional_batch(*args) == -1, (bf, bt)
    assert all(np.all(x == 7.0) for x in o)


# ---- the definition -----------------------------------------------------------------------------------------------------------

SHAPES = [(7, 3, 3, 2, 131), (7, 5, 24, 8, 300), (7, 17, 2, 1, 90), (8, 3, 1, 0, 140), (0, 1, 1, 0, 90)]


@pytest.fixture(scope="module", params=SHAPES, ids=[f"k{s[0]}Q{s[1]}D{s[2]}n{s[4]}" for s in SHAPES])
def shape(request):
    """(family, patient, theta, the functionals, their packing, the fp64 restatement) of one shape: 21 functionals, three of each kind"""
    kidx, Q, D, R, n = request.param
    fam = (kidx, Q, D, R)
    pt = synth.patient(63, n, D, n, interleave=True)
    th = synth.theta(63, n, kidx, Q, D, R)
    fs = FC.mix(n, D, pt[1], 21)
    packed = functionals.pack(fs)
    return fam, pt, th, fs, packed, FC.restate(fam, pt, th, packed)


def test_single_term_of_weight_one_is_the_posterior_point(shape):
    """point(m, t): fmean = mean and fvar = var - sigma^2 of posterior_ref.restate (the oracle's Gram matrix), 1e-12 of the largest"""
    fam, pt, th, fs, packed, _ = shape
    kidx, D = fam[0], fam[2]
    g = np.random.default_rng(5)
    m2 = g.integers(0, D, size=30).astype(np.int32)
    t2 = g.uniform(-3.0, 203.0, size=30).astype(np.float32)
    single = functionals.pack([functionals.point(int(m), float(t)) for m, t in zip(m2, t2)])
    assert np.array_equal(single[0], np.arange(31)) and np.array_equal(single[1], m2) and np.array_equal(single[2], t2) and np.all(single[3] == 1.0)
    fmean, fvar, qg = FC.restate(fam, pt, th, single)
    rm, rv, _ = PR.restate(*FC.fam_args(fam, pt), th, m2 if kidx == 7 else None, t2)
    sig2 = PR.noise_var(kidx, D, th, m2 if kidx == 7 else np.zeros(30, np.int32))
    em = float(np.abs(fmean - rm).max() / np.abs(rm).max())
    ev = float(np.abs(fvar - (rv - sig2)).max() / np.abs(rv).max())
    print(f"mean: {em:.3g}  var: {ev:.3g}")
    assert em <= 1e-12 and ev <= 1e-12


def test_general_functional_is_the_quadratic_form_of_the_joint_posterior(shape):
    """fvar = a^T (C - diag sigma^2) a and fmean = a^T mean of posterior_joint_ref.restate_joint on the functional's nodes, within
    1e-12 of sum |a_k a_l C_kl| (respectively sum |a_k mean_k|)"""
    fam, pt, th, fs, packed, (fmean, fvar, qg) = shape
    kidx, D = fam[0], fam[2]
    worst = [0.0, 0.0]
    for f, (m2, t2, a) in enumerate(fs):
        if a.shape[0] == 0:
            assert fmean[f] == 0.0 and fvar[f] == 0.0 and qg[f] == 0.0
            continue
        mean, _, Cm, _ = PJ.restate_joint(*FC.fam_args(fam, pt), th, m2 if kidx == 7 else None, t2)
        Cl = Cm - np.diag(PR.noise_var(kidx, D, th, m2 if kidx == 7 else np.zeros(len(t2), np.int32)))
        sm, sv = np.abs(a * mean).sum(), np.abs(np.outer(a, a) * Cl).sum()
        em, ev = abs(fmean[f] - a @ mean) / sm, abs(fvar[f] - a @ Cl @ a) / sv
        worst = [max(worst[0], em), max(worst[1], ev)]
        assert em <= 1e-12 and ev <= 1e-12, (f, em, ev)
    print(f"mean: {worst[0]:.3g}  var: {worst[1]:.3g}")


def test_variance_lies_between_zero_and_the_prior(shape):
    fam, pt, th, fs, packed, (fmean, fvar, qg) = shape
    assert np.all(fvar >= 0.0) and np.all(fvar <= qg)
    assert np.all(qg[[f for f, x in enumerate(fs) if x[2].shape[0] > 0]] > 0.0)


@pytest.mark.parametrize("name", list(FC.CASES))
def test_fp64_restatement_is_far_inside_the_bar(name):
    """On every input of the GPU tests the fp64 restatement and the long-double one differ by at most 0.01 x the bar of 2 fp32
    ulps of max(|ref|, 1e-3 S), in fmean and fvar: the bar then measures the device, not the reference."""
    fam, pts, th, qs = FC.case_data(name)
    worst = [0.0] * 2
    for p in FC.checked(name):
        if qs[p][0].shape[0] == 1:
            continue
        a, b = FC.case_ref(name, p), FC.case_ref(name, p, np.longdouble)
        u = FR.ulps(a, [np.asarray(x, np.float64) for x in b])
        worst = [max(x, y) for x, y in zip(worst, u)]
        assert np.all(a[1] <= a[2]), "fvar above the prior's"
    print(name, " ".join(f"{n} {x:.2g}" for n, x in zip(FR.NAMES, worst)), "(fp32 ulps)")
    assert max(worst) <= 0.01 * 2.0


def test_degenerate_contrast_is_exactly_zero_in_the_definition():
    ref = FC.case_ref("degenerate", 0)
    for k in range(3):
        assert np.all(ref[k][-FC.N_DEGENERATE:] == 0.0)


def test_far_field_limit():
    """|t_k - t| >= 5000 h: every envelope exp(-c_q tau^2) towards the data has underflowed, fmean is 0 and fvar the prior's q_g"""
    fam, pt, th, packed, qg = FC.far_case()
    assert float(packed[2].min()) < float(pt[1].min()) - 4990.0 and float(packed[2].max()) > float(pt[1].max()) + 4990.0
    assert not np.any((packed[2] > float(pt[1].min()) - 4990.0) & (packed[2] < float(pt[1].max()) + 4990.0))
    fmean, fvar, q = FC.restate(fam, pt, th, packed)
    assert np.all(fmean == 0.0) and np.array_equal(fvar, q) and np.array_equal(q, qg) and np.all(q > 0.0)
    lm, lv, lq = FC.restate(fam, pt, th, packed, dtype=np.longdouble)   # (long double does not underflow there, but nothing is left in a float)
    assert np.all(lm.astype(np.float32) == 0.0) and np.array_equal(lv.astype(np.float32), lq.astype(np.float32))
    assert np.allclose(np.asarray(lq, np.float64), qg, rtol=1e-13)


# ---- Context.functionals and medgp_amd/functionals.py ---------------------------------------------------------------------------

class _Lib:
    def medgp_functional_batch(self, *a):
        raise AssertionError("the library must not be reached")


def _bare_context(kidx, Q, D, Hn):
    ctx = object.__new__(medgp_amd.Context)    # no device: the checks under test run before the library is called
    ctx._lib, ctx._h, ctx.kernel_index, ctx.Q, ctx.D, ctx.H = _Lib(), None, kidx, Q, D, Hn
    return ctx


def test_context_functionals_argument_validation():
    ctx = _bare_context(7, 2, 3, 10)
    th = np.zeros((2, 10))
    pk = [functionals.pack([functionals.point(1, 2.0), functionals.change(0, 1.0, 7.0)]), functionals.pack([])]
    with pytest.raises(ValueError, match="theta has"):
        ctx.functionals([0, 1], np.zeros((2, 9)), pk)
    with pytest.raises(ValueError, match="packed functional lists"):
        ctx.functionals([0, 1], th, pk[:1])
    with pytest.raises(ValueError, match="expected \\(toffsets"):
        ctx.functionals([0, 1], th, [pk[0][:3], pk[1]])
    with pytest.raises(ValueError, match="required for the multi-output"):
        ctx.functionals([0, 1], th, [(pk[0][0], None, pk[0][2], pk[0][3]), pk[1]])
    with pytest.raises(ValueError, match="must start at 0"):
        ctx.functionals([0, 1], th, [(np.array([1, 3]),) + pk[0][1:], pk[1]])
    with pytest.raises(ValueError, match="must start at 0"):
        ctx.functionals([0, 1], th, [(np.array([0, 3, 1]),) + pk[0][1:], pk[1]])
    with pytest.raises(ValueError, match="for 3 terms"):
        ctx.functionals([0, 1], th, [(pk[0][0], pk[0][1], pk[0][2][:2], pk[0][3]), pk[1]])
    with pytest.raises(ValueError, match="for 2 terms"):
        ctx.functionals([0, 1], th, [(np.array([0, 1, 2]),) + pk[0][1:], pk[1]])
    with pytest.raises(ValueError, match="meta2 outside"):
        ctx.functionals([0, 1], th, [(pk[0][0], np.array([0, 3, 1]), pk[0][2], pk[0][3]), pk[1]])
    with pytest.raises(AssertionError, match="must not be reached"):   # a well-formed call does go on to the library
        ctx.functionals([0, 1], th, pk)
    with pytest.raises(AssertionError, match="must not be reached"):   # SE / SM: meta2 may be None
        _bare_context(0, 1, 1, 3).functionals([0], np.zeros((1, 3)), [(pk[0][0], None, pk[0][2], pk[0][3])])
    assert medgp_amd.functionals is functionals and "functionals" in medgp_amd.__all__


def test_builders_and_pack():
    m, t, a = functionals.point(2, 5.5)
    assert (m.dtype, t.dtype, a.dtype) == (np.int32, np.float32, np.float64)
    assert m.tolist() == [2] and t.tolist() == [5.5] and a.tolist() == [1.0]
    m, t, a = functionals.change(1, 3.0, 9.0)
    assert m.tolist() == [1, 1] and t.tolist() == [9.0, 3.0] and a.tolist() == [1.0, -1.0]
    m, t, a = functionals.contrast((0, 4.0), (2, 5.0))
    assert m.tolist() == [0, 2] and t.tolist() == [4.0, 5.0] and a.tolist() == [1.0, -1.0]
    m, t, a = functionals.combine([functionals.point(0, 1.0), functionals.change(1, 2.0, 3.0)], [0.5, -2.0])
    assert m.tolist() == [0, 1, 1] and t.tolist() == [1.0, 3.0, 2.0] and a.tolist() == [0.5, -2.0, 2.0]
    assert all(x.shape == (0,) for x in functionals.combine([]))
    toff, pm, pt_, pa = functionals.pack([functionals.point(2, 5.5), (np.zeros(0), np.zeros(0), np.zeros(0)), functionals.change(1, 3.0, 9.0)])
    assert (toff.dtype, pm.dtype, pt_.dtype, pa.dtype) == (np.int64, np.int32, np.float32, np.float64)
    assert toff.tolist() == [0, 1, 1, 3] and pm.tolist() == [2, 1, 1] and pt_.tolist() == [5.5, 9.0, 3.0] and pa.tolist() == [1.0, 1.0, -1.0]
    toff, pm, pt_, pa = functionals.pack([])
    assert toff.tolist() == [0] and pm.shape == pt_.shape == pa.shape == (0,)
    for bad in ([(np.zeros(2), np.zeros(2))], [(np.zeros(2), np.zeros(3), np.zeros(2))]):
        with pytest.raises(ValueError):
            functionals.pack(bad)
    with pytest.raises(ValueError):
        functionals.combine([functionals.point(0, 1.0)], [1.0, 2.0])


def test_window_mean_weights_sum_to_one_and_integrate_a_cubic_exactly_with_two_nodes():
    for nodes in (1, 2, 5, 25):
        m, t, a = functionals.window_mean(3, 10.0, 34.0, nodes)
        assert m.shape == t.shape == a.shape == (nodes,) and np.all(m == 3)
        assert abs(a.sum() - 1.0) <= 4e-16 * nodes and np.all(a > 0) and np.all((t > 10.0) & (t < 34.0)) and np.all(np.diff(t) > 0)
    # two nodes: exact for cubics.  On [-1, 3] the nodes 1 -+ 2 / sqrt(3) are not float32 numbers: evaluate at the rounded nodes, whose
    # offset of at most 2^-24 |t| moves the cubic by less than 1e-6
    m, t, a = functionals.window_mean(0, -1.0, 3.0, 2)
    p = np.polynomial.Polynomial([0.5, -2.0, 0.75, 1.25])
    exact = (p.integ()(3.0) - p.integ()(-1.0)) / 4.0
    nodes64 = 1.0 + 2.0 * np.array([-1.0, 1.0]) / np.sqrt(3.0)
    assert np.all(np.abs(t.astype(np.float64) - nodes64) <= 2.0 ** -24 * np.abs(nodes64))
    assert abs(a @ p(nodes64) - exact) <= 1e-14 * abs(exact)
    assert abs(a @ p(t.astype(np.float64)) - exact) <= 1e-6
    with pytest.raises(ValueError):
        functionals.window_mean(0, 1.0, 1.0, 3)
    with pytest.raises(ValueError):
        functionals.window_mean(0, 0.0, 1.0, 0)


def test_prob_above():
    p = functionals.prob_above(np.array([1.0, 1.0, 3.0, 0.0]), np.array([4.0, 4.0, 4.0, 1.0]), np.array([1.0, -1.0, 1.0, 1.6448536269514722]))
    np.testing.assert_allclose(p, [0.5, 0.8413447460685429, 0.8413447460685429, 0.05], rtol=1e-12)
    assert functionals.prob_above(2.0, 0.0, 1.0) == 1.0 and functionals.prob_above(1.0, 0.0, 1.0) == 0.5 and functionals.prob_above(0.0, 0.0, 1.0) == 0.0
    assert np.isnan(functionals.prob_above(np.nan, 1.0, 0.0)) and np.isnan(functionals.prob_above(1.0, -1e-9, 0.0)) and np.isnan(functionals.prob_above(1.0, np.nan, 0.0))
    assert 1e-200 < functionals.prob_above(np.float32(-30.0), np.float32(1.0), 0.0) < 1e-190    # the lower tail does not cancel (4.9e-198)
    assert functionals.prob_above(np.zeros((2, 3)), np.ones((2, 3)), 0.0).shape == (2, 3)
    with pytest.raises(ValueError):
        functionals.prob_above(np.zeros(2), np.zeros(3), 0.0)
