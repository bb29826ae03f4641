"""medgp_loo_batch without a GPU: the ABI surface, argument errors, the two numpy restatements of the leave-group-out
predictive distribution that the GPU tests (test_loo_gpu.py) rest on, and the condition on their inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import medgp_amd
from medgp_amd import capi
from oracle import oracle as O
import loo_cases as LC
import loo_ref as LR
from posterior_joint_ref import COND_MAX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_loo(built_lib):
    src = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    assert re.search(r"int\s+medgp_loo_batch\s*\(", src)
    lib = C.CDLL(built_lib)
    assert hasattr(lib, "medgp_loo_batch")
    assert "medgp_loo_batch" in capi.SYMBOLS
    assert capi.load().medgp_abi_version() >= 6
    lib = capi.load()
    names = [lib.medgp_profile_kernel_name(k).decode() for k in range(lib.medgp_profile_num_kernels())]
    assert {"k_loo_diag", "k_loo_gram", "k_postfactor", "k_loo_solve"} <= set(names)
    # appended: the ids of the earlier kernels did not move
    assert names[:15] == ["k_prep", "k_assemble", "k_cholinv", "k_la_step", "k_la_aux", "k_lauum", "k_gradbins", "k_wgrad", "k_epilogue",
                          "k_predict", "k_alpha", "k_posterior", "k_postcov", "k_postfactor", "k_postdraw"]
    blob = open(built_lib, "rb").read()
    assert b"k_loo_diag" in blob and b"k_loo_gram" in blob and b"k_loo_solve" in blob


def test_null_context_is_an_argument_error(built_lib):
    lib = capi.load()
    slots = np.zeros(1, np.int32)
    th = np.zeros(8)
    out = np.zeros(4, np.float32)
    rc = lib.medgp_loo_batch(None, 1, slots.ctypes.data_as(C.POINTER(C.c_int32)), th.ctypes.data_as(C.POINTER(C.c_double)), None, None,
                             out.ctypes.data_as(C.POINTER(C.c_float)), None, None, None, None, None)
    assert rc == -1   # MEDGP_ERR_ARG


def _offline_context(kidx=7, Q=2, D=3, R=2):
    """A Context object that never reached the library (no device here): enough for the checks done before the call."""
    ctx = medgp_amd.Context.__new__(medgp_amd.Context)
    ctx._lib, ctx._h = capi.load(), None
    ctx.kernel_index, ctx.Q, ctx.D, ctx.R, ctx.device = kidx, Q, D, R, 0
    ctx.H = O.num_hyp(kidx, Q, D, R)
    ctx._slot_n, ctx._slot_meta = {}, {}
    ctx._remember(0, np.array([0, 1, 2], np.int32), 3)
    ctx._remember(1, np.array([2], np.int32), 1)
    return ctx


@pytest.mark.parametrize("case", ["theta", "npatients", "length", "dtype", "below", "unknown_slot", "scheme", "no_patient", "meta_range"])
def test_loo_rejects_mismatched_inputs(built_lib, case):
    ctx = _offline_context()
    slots = [0, 1]
    th = np.zeros((2, ctx.H))
    groups = [np.array([0, 1, -1], np.int32), np.array([0], np.int32)]
    if case == "theta":
        th = th[:, :-1]
    elif case == "npatients":
        groups = groups[:1]
    elif case == "length":
        groups = [np.array([0, 1], np.int32), np.array([0], np.int32)]
    elif case == "dtype":
        groups = [np.array([0.0, 1.0, 2.0]), np.array([0], np.int32)]
    elif case == "below":
        groups = [np.array([0, -2, 1], np.int32), np.array([0], np.int32)]
    elif case == "unknown_slot":
        slots = [0, 5]
    elif case == "scheme":
        groups = "window"
    elif case == "no_patient":
        slots, th, groups = [], np.zeros((0, ctx.H)), []
    elif case == "meta_range":
        ctx._remember(1, np.array([3], np.int32), 1)   # a covariate beyond D
        groups = "covariate"
    with pytest.raises(ValueError):
        ctx.loo(slots, th, groups)


def test_loo_args_lay_out_the_call(built_lib):
    ctx = _offline_context()
    th = np.zeros((2, ctx.H))
    slots, theta, ns, gs, ng = ctx._loo_args([0, 1], th, None)
    assert ns == [3, 1] and gs is None and ng is None
    slots, theta, ns, gs, ng = ctx._loo_args([0, 1], th, "covariate")
    assert list(ng) == [3, 3] and list(gs[0]) == [0, 1, 2] and list(gs[1]) == [2]
    slots, theta, ns, gs, ng = ctx._loo_args([1, 0], th, [np.array([-1]), np.array([4, -1, 4])])
    assert list(ng) == [0, 5] and gs[1].dtype == np.int32


# ---------------------------------------------------------------------------------------------------------------------------
# the two restatements
# ---------------------------------------------------------------------------------------------------------------------------
def test_refit_of_singletons_is_the_textbook_formula():
    """Rasmussen & Williams (5.10)-(5.12): mu_i = y_i - [K^-1 y]_i / [K^-1]_ii, var_i = 1 / [K^-1]_ii"""
    pts, th, _, _ = LC.case_data(0)
    p = 5
    args = LC.family_args(LC.CASES[0][:4], pts[p])
    K = LR.gram(*args[:6], th[p])
    y = pts[p][2].astype(np.float64)
    Ki = np.linalg.inv(K)
    mean, var, lpd, total = LR.refit(*args, th[p])
    d = np.diag(Ki)
    assert np.allclose(mean, y - (Ki @ y) / d, rtol=1e-9, atol=1e-12) and np.allclose(var, 1.0 / d, rtol=1e-9)
    ref_lpd = -0.5 * np.log(var) - (y - mean) ** 2 / (2.0 * var) - 0.5 * np.log(2.0 * O.REF_PI)
    assert np.allclose(lpd, ref_lpd, rtol=1e-9, atol=1e-12) and np.isclose(total, ref_lpd.sum(), rtol=1e-12)


def test_refit_of_one_group_of_everything_is_the_prior():
    pts, th, _, _ = LC.case_data(1)
    p = 4
    args = LC.family_args(LC.CASES[1][:4], pts[p])
    n = pts[p][1].shape[0]
    mean, var, lpd, total = LR.refit(*args, th[p], np.zeros(n, np.int32), 1)
    K = LR.gram(*args[:6], th[p])
    ref = O.nlml_grad(*args, th[p], flag_grad=False)
    assert np.all(mean == 0.0) and np.array_equal(var, np.diag(K))
    assert abs(lpd[0] + ref["nlml"]) <= 1e-10 * abs(ref["nlml"]) and total == lpd[0]


def test_refit_conventions():
    """-1 is never held out (NaN mean / var, still conditioned on); an empty group has lpd 0.0; jitter rounds add the noise"""
    pts, th, _, _ = LC.case_data(5)
    args = LC.family_args(LC.CASES[5][:4], pts[1])
    n = pts[1][1].shape[0]
    ids = np.full(n, -1, np.int32)
    ids[[3, 10, 11]] = [0, 2, 2]
    mean, var, lpd, total = LR.refit(*args, th[1], ids, 4)
    assert np.isnan(mean[ids < 0]).all() and np.isnan(var[ids < 0]).all() and not np.isnan(mean[ids >= 0]).any()
    assert lpd[1] == 0.0 and lpd[3] == 0.0 and lpd[0] != 0.0 and total == lpd.sum()
    one = LR.refit(*args, th[1])
    assert mean[3] == one[0][3] and var[3] == one[1][3] and lpd[0] == one[2][3]   # the same conditioning set
    v0, v2 = LR.refit(*args, th[1])[1], LR.refit(*args, th[1], jitter_rounds=2)[1]
    assert np.all(v2 > v0)
    with pytest.raises(AssertionError):
        LR.refit(*args, th[1], np.full(n, 4, np.int32), 4)


@pytest.mark.parametrize("i", range(len(LC.CASES)), ids=[LC.case_id(s) for s in LC.CASES])
def test_inputs_are_well_conditioned_and_the_restatements_agree(i):
    """cond(K) <= 1e4 for every input of the GPU tests, and the inverse identity within 1/8 of the GPU bar of the refit: the
    bar cannot be met or missed by the choice of reference"""
    pts, th, gs, ngs = LC.case_data(i)
    for p, pt in enumerate(pts):
        args = LC.family_args(LC.CASES[i][:4], pt)
        assert LR.cond(LR.gram(*args[:6], th[p])) <= COND_MAX
        LR.check_loo(LC.case_ref(i, p), pt[2], LR.via_inverse(*args, th[p], gs[p], ngs[p]), scale=1.0 / 8.0)


def test_the_other_inputs_are_well_conditioned():
    for fam, pts, th, gs in (LC.jitter_case(), LC.invariance_case()):
        for p, pt in enumerate(pts):
            args = LC.family_args(fam, pt)
            assert LR.cond(LR.gram(*args[:6], th[p])) <= COND_MAX
            assert gs[p].shape == pt[1].shape and gs[p].min() >= 0
    kinds = {s[5] for s in LC.CASES}
    assert kinds == {"null", "covariate", "window", "random5", "all", "minus", "mixed"}
    # an unobserved covariate (an empty group), -1 entries, and singletons beside larger groups are really there
    assert any(np.bincount(g, minlength=ng).min() == 0 for i, s in enumerate(LC.CASES) if s[5] == "covariate" for g, ng in zip(*LC.case_data(i)[2:]))
    assert all((g < 0).any() for i, s in enumerate(LC.CASES) if s[5] == "minus" for g in LC.case_data(i)[2] if g.size > 3)
    for i, s in enumerate(LC.CASES):
        if s[5] == "mixed":
            for g in LC.case_data(i)[2]:
                if g.size > 10:
                    cnt = np.bincount(g)
                    assert (cnt == 1).any() and (cnt > 64).any() or g.size < 140


def test_check_loo_has_teeth():
    pts, th, gs, ngs = LC.case_data(5)
    ref = LC.case_ref(5, 0)
    y = pts[0][2]
    good = (ref[0].astype(np.float32), ref[1].astype(np.float32), ref[2].copy(), ref[3])
    LR.check_loo(ref, y, good)
    for k, f in ((0, lambda a: a * np.float32(1 + 2.0 ** -20)), (1, lambda a: a * np.float32(1 + 2.0 ** -20)), (2, lambda a: a * (1 + 1e-9)),
                 (1, lambda a: -a), (0, lambda a: np.where(np.arange(a.shape[0]) == 2, np.nan, a).astype(np.float32))):
        bad = list(good)
        bad[k] = f(good[k])
        with pytest.raises(AssertionError):
            LR.check_loo(ref, y, tuple(bad))
    with pytest.raises(AssertionError):
        LR.check_loo(ref, y, good[:3] + (ref[3] * (1 + 1e-9) + 1e-9,))
