"""medgp_functional_joint_batch without a GPU: the ABI surface and the argument errors that need no device; the definition
(functional_joint_ref.py) held against what exists -- its fp64 restatement against the long-double one on every input of the GPU tests
(functional_cases.py), its diagonal against functional_ref's fvar, the whole block against A^T (C - diag sigma^2) A of
posterior_joint_ref; medgp_amd/design.py against the definition BY REFIT (the variance of a target after a candidate is appended to the
training set), with greedy against brute force and the edge cases; Context.functionals_joint's argument checks."""
import ctypes as C
import itertools
import json
import os
import re

import numpy as np
import pytest

import medgp_amd
from medgp_amd import capi, design, functionals
import functional_cases as FC
import functional_joint_ref as FJ
import functional_ref as FR
import posterior_joint_ref as PJ
import posterior_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "design_refit_spread.json")


def test_header_declares_and_library_exports_functional_joint(built_lib):
    src = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    assert re.search(r"int\s+medgp_functional_joint_batch\s*\(", src)
    doc = src[src.index("JOINT posterior of a patient's linear functionals"):src.index("int medgp_functional_joint_batch")]
    for ref in ("core/gp_regression.cpp:128-214", "kernel/c_kernel_LMC_SM.cpp:329-372", "tests/functional_joint_ref.py", "2 fp32 ulps",
                "no clamp", "BIT FOR BIT", "exactly symmetric", "REORDERING", "SWAPPING THE ORDER", "MEDGP_ERR_CAPACITY", "slope terms",
                "sampling", "rectangular"):
        assert ref in doc, ref
    assert hasattr(C.CDLL(built_lib), "medgp_functional_joint_batch")
    assert "medgp_functional_joint_batch" in capi.SYMBOLS
    lib = capi.load()
    assert lib.medgp_abi_version() >= 12
    # the kernel has no profile entry of its own (k_funccov is accounted under k_postcov), but it is in the library
    names = [lib.medgp_profile_kernel_name(k).decode() for k in range(lib.medgp_profile_num_kernels())]
    assert len(names) == 23 and "k_postcov" in names
    assert not any("functional" in n or "funccov" in n for n in names)
    assert b"k_funccov" in open(built_lib, "rb").read()


def test_null_context_and_null_or_broken_arguments_are_argument_errors(built_lib):
    """The argument checks run before any device work; without a context (and so without a device) every call is MEDGP_ERR_ARG."""
    lib = capi.load()
    i32, i64, f32, f64 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))), \
        (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    slots, th, st = np.zeros(1, np.int32), np.zeros(8), np.zeros(1, np.int32)
    foff, toff = np.array([0, 2], np.int64), np.array([0, 1, 3], np.int64)
    m2, t2, a = np.zeros(3, np.int32), np.zeros(3, np.float32), np.ones(3)
    o = [np.full(2, 7.0, np.float32), np.full(2, 7.0, np.float32), np.full(4, 7.0, np.float32)]
    full = [None, 1, i32(slots), f64(th), i64(foff), i64(toff), i32(m2), f32(t2), f64(a), f32(o[0]), f32(o[1]), f32(o[2]), i32(st)]
    assert lib.medgp_functional_joint_batch(*full) == -1   # MEDGP_ERR_ARG
    for drop in range(2, 13):
        args = list(full)
        args[drop] = None
        assert lib.medgp_functional_joint_batch(*args) == -1, drop
    for bf, bt in (([1, 2], [0, 1, 3]), ([0, -1], [0, 1, 3]), ([0, 2], [1, 1, 3]), ([0, 2], [0, 3, 1])):
        args = list(full)
        args[4], args[5] = i64(np.array(bf, np.int64)), i64(np.array(bt, np.int64))
        assert lib.medgp_functional_joint_batch(*args) == -1, (bf, bt)
    assert all(np.all(x == 7.0) for x in o)


# ---- the definition -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(FC.CASES))
def test_fp64_restatement_is_far_inside_the_bar(name):
    """On every input of the GPU tests the fp64 restatement and the long-double one differ by at most 0.01 x the bar of 2 fp32 ulps of
    max(|ref|, 1e-3 S) in fmean, fvar and fcov (S of fcov over the patient's whole block): the bar then measures the device, not the
    reference.  The diagonal of fcov is held to functional_ref's fvar (another summation order of the same quantity) at the same
    0.01 x bar."""
    fam, pts, th, qs = FC.case_data(name)
    worst, wdiag = [0.0] * 3, 0.0
    for p in FC.checked(name):
        if qs[p][0].shape[0] == 1:
            continue
        a, b = FJ.case_ref(name, p), FJ.case_ref(name, p, np.longdouble)
        worst = [max(x, y) for x, y in zip(worst, FJ.ulps(a, [np.asarray(x, np.float64) for x in b]))]
        assert np.array_equal(a[2], a[2].T) and np.array_equal(np.diag(a[2]), a[1])
        wdiag = max(wdiag, PR.ulp_error(a[1], FC.case_ref(name, p)[1]))
    print(name, " ".join(f"{n} {x:.2g}" for n, x in zip(FJ.NAMES, worst)), f"diag vs functional_ref {wdiag:.2g} (fp32 ulps)")
    assert max(worst) <= 0.01 * 2.0 and wdiag <= 0.01 * 2.0


def test_degenerate_and_empty_functionals_have_exactly_zero_rows_in_the_definition():
    ref = FJ.case_ref("degenerate", 0)
    toff = FC.case_data("degenerate")[3][0][0]
    empty = np.flatnonzero(np.diff(toff) == 0)
    assert empty.size > 0
    for idx in (empty, np.arange(ref[0].shape[0] - FC.N_DEGENERATE, ref[0].shape[0])):
        assert np.all(ref[2][idx] == 0.0) and np.all(ref[2][:, idx] == 0.0) and np.all(ref[3][idx] == 0.0)


@pytest.mark.parametrize("shape", [(7, 3, 3, 2, 131), (0, 1, 1, 0, 90)], ids=["lmc_sm", "se"])
def test_definition_is_the_quadratic_form_of_the_joint_posterior(shape):
    """fcov = A^T (C - diag sigma^2) A with C of posterior_joint_ref.restate_joint (the oracle's Gram matrix) at the terms of all
    functionals, every element within 1e-12 of sum_kl |a_k a_l C_kl| (the tolerance test_functional.py uses for the variance)"""
    kidx, Q, D, R, n = shape
    fam = (kidx, Q, D, R)
    pt = medgp_amd.synth.patient(63, n, D, n, interleave=True)
    th = medgp_amd.synth.theta(63, n, kidx, Q, D, R)
    toff, m2, t2, a = functionals.pack(FC.mix(n, D, pt[1], 21))
    fmean, fvar, fcov, _ = FJ.restate_case(fam, pt, th, (toff, m2, t2, a))
    mean, _, Cm, _ = PJ.restate_joint(*FC.fam_args(fam, pt), th, m2 if kidx == 7 else None, t2)
    Cl = Cm - np.diag(PR.noise_var(kidx, D, th, m2 if kidx == 7 else np.zeros(len(t2), np.int32)))
    A = np.zeros((len(t2), len(toff) - 1))
    for f in range(len(toff) - 1):
        A[toff[f]:toff[f + 1], f] = a[toff[f]:toff[f + 1]]
    scale = np.abs(A).T @ np.abs(Cl) @ np.abs(A)
    live = scale > 0
    assert np.all(fcov[~live] == 0.0) and live.sum() > 300
    err = float((np.abs(fcov - A.T @ Cl @ A)[live] / scale[live]).max())
    em = float((np.abs(fmean - A.T @ mean) / np.maximum(np.abs(A).T @ np.abs(mean), 1e-300)).max())
    print(f"fcov: {err:.3g}  fmean: {em:.3g}")
    assert err <= 1e-12 and em <= 1e-12


# ---- medgp_amd/design.py against the definition, by refit ---------------------------------------------------------------------------

def _design_case():
    """One LMC-SM patient (parity_d3's first: n = 70, D = 3) with three targets -- a 24 h mean, a 6 h change, a point -- and a grid of
    3 covariates x 7 times as candidates, in one list of functionals"""
    fam, pts, th, _ = FC.case_data("parity_d3")
    pt, th = pts[0], th[0]
    lo, hi = float(pt[1].min()), float(pt[1].max())
    targets = [functionals.window_mean(0, lo + 10.0, lo + 34.0, 25), functionals.change(1, hi - 6.0, hi), functionals.point(2, 0.5 * (lo + hi))]
    times = np.linspace(lo + 2.0, hi + 2.0, 7).astype(np.float32)
    cands = design.candidates(range(3), times)
    return fam, pt, th, targets, cands


def _refit_var(fam, pt, th, targets, extra, dtype):
    """fvar of the targets after the measurements `extra` (point functionals) joined the training set: functional_ref.restate on
    n + len(extra) observations (their values do not matter to the variance)"""
    meta = np.concatenate([pt[0]] + [e[0] for e in extra]).astype(np.int32)
    t = np.concatenate([pt[1]] + [e[1] for e in extra]).astype(np.float32)
    y = np.concatenate([pt[2], np.zeros(len(extra), np.float32)]).astype(np.float32)
    return FC.restate(fam, (meta, t, y), th, functionals.pack(targets), dtype=dtype)[1]


def _refit_spreads(dtype):
    """(single, double): max |refit - downdate| / q_g over the targets, for every single candidate and for three pairs of candidates,
    both sides in dtype (the downdate written out here; design.py is float64)"""
    fam, pt, th, targets, cands = _design_case()
    nt, nc = len(targets), len(cands)
    _, _, cov, Qp = FJ.restate_case(fam, pt, th, functionals.pack(targets + cands), dtype=dtype)
    qg = np.diag(Qp)[:nt]
    noise = design.noise_variance(fam[0], fam[2], th, [c[0][0] for c in cands]).astype(dtype)
    T = np.arange(nt)
    single = 0.0
    for c in range(nc):
        down = cov[T, T] - cov[T, nt + c] ** 2 / (cov[nt + c, nt + c] + noise[c])
        single = max(single, float((np.abs(_refit_var(fam, pt, th, targets, [cands[c]], dtype) - down) / qg).max()))
    double = 0.0
    for c, d in PAIRS:
        c1 = cov - np.outer(cov[:, nt + c], cov[:, nt + c]) / (cov[nt + c, nt + c] + noise[c])
        c2 = c1 - np.outer(c1[:, nt + d], c1[:, nt + d]) / (c1[nt + d, nt + d] + noise[d])
        double = max(double, float((np.abs(_refit_var(fam, pt, th, targets, [cands[c], cands[d]], dtype) - c2[T, T]) / qg).max()))
    return single, double


PAIRS = ((0, 10), (3, 4), (20, 7))
REFIT_FACTOR = 50.0   # the rule of forecast_lpd_spread.json: two fp64 programs may differ between numpy builds by a summation-order factor


def _refit_bound():
    return REFIT_FACTOR * float(json.load(open(GOLDEN))["spread_fp64"])


def test_refit_spread_is_recorded():
    """The identity design.py rests on -- the variance after a measurement is the rank-1 downdate of the joint covariance -- holds to
    rounding: written out in long double the refit and the downdate agree far closer than in fp64.  The fp64 spread, relative to the
    target's prior variance q_g, is recorded in tests/golden/design_refit_spread.json (MEDGP_RECORD_GOLDEN=1 rewrites it); 50 x that
    figure is the tolerance of the design tests below."""
    s64, s80 = _refit_spreads(np.float64), _refit_spreads(np.longdouble)
    print(f"refit spread / q_g: fp64 {max(s64):.3g}  long double {max(s80):.3g}")
    if os.environ.get("MEDGP_RECORD_GOLDEN") == "1":
        json.dump({"case": "parity_d3 patient 0, 3 targets, 21 candidates, pairs " + str(list(PAIRS)), "spread_fp64": max(s64),
                   "spread_longdouble": max(s80),
                   "what": "max |fvar after refit on n + 1 (n + 2) observations - rank-1 downdate(s) of fcov| / q_g (tests/test_functional_joint.py)"},
                  open(GOLDEN, "w"), indent=1)
    rec = json.load(open(GOLDEN))
    assert 0.0 < rec["spread_fp64"] < 1e-9
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        assert max(s80) <= rec["spread_fp64"]
    assert max(s64) <= _refit_bound(), (s64, rec["spread_fp64"])


@pytest.fixture(scope="module")
def dcase():
    fam, pt, th, targets, cands = _design_case()
    nt, nc = len(targets), len(cands)
    _, _, cov, Qp = FJ.restate_case(fam, pt, th, functionals.pack(targets + cands))
    noise = design.noise_variance(fam[0], fam[2], th, [c[0][0] for c in cands])
    return fam, pt, th, targets, cands, cov, np.diag(Qp)[:nt], noise, np.arange(nt), nt + np.arange(nc)


def test_variance_reduction_and_condition_against_refit(dcase):
    fam, pt, th, targets, cands, cov, qg, noise, T, Cn = dcase
    vr = design.variance_reduction(cov, T, Cn, noise)
    assert vr.shape == (len(T), len(Cn)) and np.all(vr >= 0.0) and np.all(vr <= cov[T, T][:, None])
    worst = 0.0
    for c in range(len(Cn)):
        worst = max(worst, float((np.abs(_refit_var(fam, pt, th, targets, [cands[c]], np.float64) - (cov[T, T] - vr[:, c])) / qg).max()))
    for c, d in PAIRS:
        after = design.condition(cov, [Cn[c], Cn[d]], [noise[c], noise[d]])
        assert after.shape == cov.shape and np.allclose(after, after.T, rtol=0, atol=1e-15 * np.abs(cov).max())
        worst = max(worst, float((np.abs(_refit_var(fam, pt, th, targets, [cands[c], cands[d]], np.float64) - after[T, T]) / qg).max()))
        one = design.condition(cov, [Cn[c]], [noise[c]])   # one pick is variance_reduction's column
        assert np.allclose(one[T, T], cov[T, T] - vr[:, c], rtol=1e-14, atol=0)
    print(f"refit vs design.py: {worst:.3g} of q_g (bound {_refit_bound():.3g})")
    assert worst <= _refit_bound()
    assert np.array_equal(design.condition(cov, [], []), cov)


def test_greedy_against_brute_force(dcase):
    fam, pt, th, targets, cands, cov, qg, noise, T, Cn = dcase
    tol = 1e-12 * float(cov[T, T].sum())
    for w in (None, np.array([5.0, 0.25, 1.0])):
        ww = np.ones(len(T)) if w is None else w
        total = lambda cv: float(ww @ cv[T, T])
        # k = 1: the pick is the best single candidate
        picks, sums = design.greedy(cov, T, Cn, noise, 1, w)
        singles = [total(design.condition(cov, [Cn[c]], [noise[c]])) for c in range(len(Cn))]
        assert picks.shape == (1,) and picks.dtype == np.int64 and abs(sums[0] - min(singles)) <= tol and abs(singles[picks[0]] - min(singles)) <= tol
        # k = 2: on this case the greedy pair is the best pair
        picks, sums = design.greedy(cov, T, Cn, noise, 2, w)
        pairs = {(c, d): total(design.condition(cov, [Cn[c], Cn[d]], [noise[c], noise[d]])) for c, d in itertools.combinations(range(len(Cn)), 2)}
        assert picks[0] != picks[1] and sums[1] < sums[0] < total(cov)
        assert abs(sums[1] - pairs[tuple(sorted(picks.tolist()))]) <= tol
        assert sums[1] <= min(pairs.values()) + tol, (picks, sums, min(pairs, key=pairs.get), min(pairs.values()))
    # the weights are honoured: all weight on one target picks that target's best candidate
    for t in range(len(T)):
        w = np.zeros(len(T))
        w[t] = 1.0
        picks, _ = design.greedy(cov, T, Cn, noise, 1, w)
        vr = design.variance_reduction(cov, T, Cn, noise)
        assert vr[t, picks[0]] == vr[t].max()
    # every candidate at most once, all of them when k = the number of candidates, and the sums only fall
    picks, sums = design.greedy(cov, T, Cn, noise, len(Cn))
    assert sorted(picks.tolist()) == list(range(len(Cn))) and np.all(np.diff(sums) <= 0.0)


def test_design_edge_cases():
    cov = np.array([[2.0, 1.0, 0.0, 0.5], [1.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.5, 0.0, 0.0, 1.0]])
    # a candidate the data determine, measured without noise: NaN, never infinity; with noise: a reduction of 0
    vr = design.variance_reduction(cov, [0], [1, 2, 3], [0.0, 0.0, 1.0])
    assert vr.shape == (1, 3) and vr[0, 0] == 1.0 and np.isnan(vr[0, 1]) and vr[0, 2] == 0.125 and not np.any(np.isinf(vr))
    assert np.isnan(design.variance_reduction(cov, [0], [2], [-1.0])[0, 0])
    assert design.variance_reduction(cov, [0], [2], [1.0])[0, 0] == 0.0
    assert design.variance_reduction(cov, [], [1], [0.0]).shape == (0, 1) and design.variance_reduction(cov, [0], [], []).shape == (1, 0)
    assert np.all(np.isnan(design.variance_reduction(np.full((2, 2), np.nan), [0], [1], [1.0])))   # a failed patient
    # greedy never picks the zero-variance candidate and never one twice; more picks than usable candidates raise
    picks, sums = design.greedy(cov, [0], [1, 2, 3], [0.0, 0.0, 1.0], 2)
    assert picks.tolist() == [0, 2] and sums[0] == 1.0
    with pytest.raises(ValueError, match="picks possible"):
        design.greedy(cov, [0], [1, 2, 3], [0.0, 0.0, 1.0], 3)
    with pytest.raises(ValueError, match="not positive"):
        design.condition(cov, [2], [0.0])
    twice = design.condition(cov, [3, 3], [1.0, 1.0])   # a repeated measurement is allowed in condition
    assert abs(twice[3, 3] - 1.0 / 3.0) <= 1e-15
    # shapes
    for bad in (lambda: design.variance_reduction(np.zeros((2, 3)), [0], [1], [0.0]), lambda: design.variance_reduction(cov, [0], [1, 2], [0.0]),
                lambda: design.variance_reduction(cov, [4], [1], [0.0]), lambda: design.variance_reduction(cov, [0], [-1], [0.0]),
                lambda: design.variance_reduction(cov, [[0]], [1], [0.0]), lambda: design.condition(cov, [1, 2], [0.0]),
                lambda: design.greedy(cov, [0], [1, 3], [0.0, 0.0], 1, weights=[1.0, 2.0]), lambda: design.greedy(cov, [0], [1, 3], [0.0, 0.0], 3),
                lambda: design.greedy(cov, [0], [1, 3], [0.0, 0.0], -1), lambda: design.noise_variance(7, 2, np.zeros(9), [2])):
        with pytest.raises(ValueError):
            bad()
    # noise_variance: the likelihood hypers are log sigma; SE / SM have one
    th = np.log(np.array([0.5, 2.0, 3.0, 9.0]))
    assert np.allclose(design.noise_variance(7, 3, th, [2, 0, 0]), [9.0, 0.25, 0.25], rtol=1e-15)
    assert np.allclose(design.noise_variance(0, 1, th, [0, 0]), [0.25, 0.25], rtol=1e-15)
    assert np.array_equal(design.noise_variance(7, 3, th, [1]), PR.noise_var(7, 3, th, [1]))
    c = design.candidates([1, 0], [2.0, 3.5, 7.0])
    assert len(c) == 6 and [(int(x[0][0]), float(x[1][0])) for x in c] == [(1, 2.0), (1, 3.5), (1, 7.0), (0, 2.0), (0, 3.5), (0, 7.0)]
    assert all(x[2].tolist() == [1.0] for x in c)
    assert medgp_amd.design is design and "design" in medgp_amd.__all__
    for fn in (design.variance_reduction, design.condition, design.greedy):
        assert fn.__doc__
    assert "K + k diag(sigma^2)" in design.__doc__ and "caller" in design.__doc__


# ---- Context.functionals_joint ------------------------------------------------------------------------------------------------

class _Lib:
    def medgp_functional_joint_batch(self, *a):
        raise AssertionError("the library must not be reached")


def _bare_context(kidx, Q, D, Hn):
    ctx = object.__new__(medgp_amd.Context)    # no device: the checks under test run before the library is called
    ctx._lib, ctx._h, ctx.kernel_index, ctx.Q, ctx.D, ctx.H = _Lib(), None, kidx, Q, D, Hn
    return ctx


def test_context_functionals_joint_argument_validation():
    ctx = _bare_context(7, 2, 3, 10)
    th = np.zeros((2, 10))
    pk = [functionals.pack([functionals.point(1, 2.0), functionals.change(0, 1.0, 7.0)]), functionals.pack([])]
    with pytest.raises(ValueError, match="theta has"):
        ctx.functionals_joint([0, 1], np.zeros((2, 9)), pk)
    with pytest.raises(ValueError, match="packed functional lists"):
        ctx.functionals_joint([0, 1], th, pk[:1])
    with pytest.raises(ValueError, match="expected \\(toffsets"):
        ctx.functionals_joint([0, 1], th, [pk[0][:3], pk[1]])
    with pytest.raises(ValueError, match="required for the multi-output"):
        ctx.functionals_joint([0, 1], th, [(pk[0][0], None, pk[0][2], pk[0][3]), pk[1]])
    with pytest.raises(ValueError, match="must start at 0"):
        ctx.functionals_joint([0, 1], th, [(np.array([1, 3]),) + pk[0][1:], pk[1]])
    with pytest.raises(ValueError, match="must start at 0"):
        ctx.functionals_joint([0, 1], th, [(np.array([0, 3, 1]),) + pk[0][1:], pk[1]])
    with pytest.raises(ValueError, match="for 3 terms"):
        ctx.functionals_joint([0, 1], th, [(pk[0][0], pk[0][1], pk[0][2][:2], pk[0][3]), pk[1]])
    with pytest.raises(ValueError, match="meta2 outside"):
        ctx.functionals_joint([0, 1], th, [(pk[0][0], np.array([0, 3, 1]), pk[0][2], pk[0][3]), pk[1]])
    with pytest.raises(AssertionError, match="must not be reached"):   # a well-formed call does go on to the library
        ctx.functionals_joint([0, 1], th, pk)
    with pytest.raises(AssertionError, match="must not be reached"):   # SE / SM: meta2 may be None
        _bare_context(0, 1, 1, 3).functionals_joint([0], np.zeros((1, 3)), [(pk[0][0], None, pk[0][2], pk[0][3])])
