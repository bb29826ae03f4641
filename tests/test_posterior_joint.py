"""medgp_posterior_joint_batch without a GPU: the ABI surface, argument errors, the numpy restatement of the joint posterior
that the GPU tests (test_posterior_joint_gpu.py) hold the device to, the condition on their inputs, and the checker's teeth."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import medgp_amd
from medgp_amd import capi, synth
from oracle import oracle as O
import posterior_joint_cases as PC
from posterior_joint_ref import COND_MAX, check_joint, cond, draw, restate_joint
from posterior_ref import noise_var, restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_posterior_joint(built_lib):
    src = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    assert re.search(r"int\s+medgp_posterior_joint_batch\s*\(", src)
    lib = C.CDLL(built_lib)
    assert hasattr(lib, "medgp_posterior_joint_batch")
    assert "medgp_posterior_joint_batch" in capi.SYMBOLS
    assert capi.load().medgp_abi_version() >= 5
    blob = open(built_lib, "rb").read()
    assert b"k_postcov" in blob and b"k_postfactor" in blob and b"k_postdraw" in blob
    names = [lib_name.decode() for lib_name in _kernel_names()]
    assert {"k_postcov", "k_postfactor", "k_postdraw"} <= set(names)


def _kernel_names():
    lib = capi.load()
    return [lib.medgp_profile_kernel_name(k) for k in range(lib.medgp_profile_num_kernels())]


def test_null_context_is_an_argument_error(built_lib):
    lib = capi.load()
    off = np.zeros(2, np.int64)
    slots = np.zeros(1, np.int32)
    th = np.zeros(8)
    rc = lib.medgp_posterior_joint_batch(None, 1, slots.ctypes.data_as(C.POINTER(C.c_int32)), th.ctypes.data_as(C.POINTER(C.c_double)),
                                         off.ctypes.data_as(C.POINTER(C.c_int64)), None, None, 0, None, None, None, None, None, None, None)
    assert rc == -1   # MEDGP_ERR_ARG


def _offline_context(kidx=7, Q=2, D=3, R=2):
    """A Context object that never reached the library (no device here): enough for the checks done before the call."""
    ctx = medgp_amd.Context.__new__(medgp_amd.Context)
    ctx._lib, ctx._h = capi.load(), None
    ctx.kernel_index, ctx.Q, ctx.D, ctx.R, ctx.device = kidx, Q, D, R, 0
    ctx.H = O.num_hyp(kidx, Q, D, R)
    return ctx


@pytest.mark.parametrize("case", ["theta", "npatients", "nmeta", "ragged", "meta_missing", "neps", "eps_rows", "eps_1d", "eps_widths",
                                  "eps_empty", "nothing"])
def test_posterior_joint_rejects_mismatched_inputs(built_lib, case):
    ctx = _offline_context()
    th = np.zeros((2, ctx.H))
    m2 = [np.zeros(3, np.int32), np.zeros(1, np.int32)]
    t2 = [np.zeros(3, np.float32), np.zeros(1, np.float32)]
    eps = [np.zeros((3, 4)), np.zeros((1, 4))]
    cov = True
    if case == "theta":
        th = th[:, :-1]
    elif case == "npatients":
        t2 = t2[:1]
    elif case == "nmeta":
        m2 = m2[:1]
    elif case == "ragged":
        m2 = [np.zeros(2, np.int32), np.zeros(1, np.int32)]
    elif case == "meta_missing":
        m2 = None
    elif case == "neps":
        eps = eps[:1]
    elif case == "eps_rows":
        eps = [np.zeros((2, 4)), np.zeros((1, 4))]
    elif case == "eps_1d":
        eps = [np.zeros(3), np.zeros(1)]
    elif case == "eps_widths":
        eps = [np.zeros((3, 4)), np.zeros((1, 5))]
    elif case == "eps_empty":
        eps = [np.zeros((3, 0)), np.zeros((1, 0))]
    elif case == "nothing":
        eps, cov = None, False
    with pytest.raises(ValueError):
        ctx.posterior_joint([0, 1], th, m2, t2, eps, cov=cov)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
FAMILIES = [(7, 3, 3, 2, 70), (7, 5, 24, 8, 300), (7, 9, 2, 1, 90), (8, 3, 1, 0, 50), (0, 1, 1, 0, 40)]


def _family_case(kidx, Q, D, R, n, m=60, seed=31):
    meta, t, y = synth.patient(seed, 0, D, n, interleave=True)
    th = synth.theta(seed, 0, kidx, Q, D, R)
    m2, t2 = PC.grid(np.random.default_rng(seed), D, m)
    mi, m2i = (meta, m2) if kidx == 7 else (None, None)
    return (kidx, Q, D, R, mi, t, y, th, m2i, t2)


@pytest.mark.parametrize("kidx,Q,D,R,n", FAMILIES)
@pytest.mark.parametrize("k", [0, 2])
def test_restatement_diagonal_is_the_marginal_variance(kidx, Q, D, R, n, k):
    case = _family_case(kidx, Q, D, R, n)
    mean, var, C, Lc = restate_joint(*case, jitter_rounds=k)
    rm, rv, _ = restate(*case, jitter_rounds=k)
    np.testing.assert_allclose(np.diag(C), rv, rtol=1e-12, atol=1e-12 * np.abs(rv).max())
    np.testing.assert_allclose(var, rv, rtol=1e-12, atol=1e-12 * np.abs(rv).max())
    np.testing.assert_allclose(mean, rm, rtol=1e-9, atol=1e-10 * np.abs(rm).max())
    # symmetric positive definite, bounded below by the smallest noise variance
    assert np.array_equal(C, C.T)
    sig2 = noise_var(kidx, D, case[7], case[8] if kidx == 7 else np.zeros(len(case[9]), np.int32))
    assert np.linalg.eigvalsh(C)[0] >= sig2.min() * (1.0 - 1e-9)
    np.testing.assert_allclose(Lc @ Lc.T, C, rtol=0, atol=1e-12 * np.abs(C).max())
    assert np.all(np.triu(Lc, 1) == 0.0)


@pytest.mark.parametrize("kidx,Q,D,R,n", FAMILIES)
def test_far_block_has_the_prior_covariance(kidx, Q, D, R, n):
    """test points further than ten of the longest length scales from every observation: their block of C is the prior Gram"""
    kidx_, Q_, D_, R_, mi, t, y, th, m2i, t2 = _family_case(kidx, Q, D, R, n)
    g = np.random.default_rng(5)
    far = g.uniform(5000.0, 5100.0, size=25).astype(np.float32)   # length scales of synth.theta are at most 72 h
    t2 = np.concatenate([t2, far])
    if kidx == 7:
        m2i = np.concatenate([m2i, g.integers(0, D, size=25).astype(np.int32)])
    _, _, C, _ = restate_joint(kidx, Q, D, R, mi, t, y, th, m2i, t2)
    prior = O.gram(kidx, Q, D, R, m2i[-25:] if kidx == 7 else None, far, th)
    assert np.abs(C[-25:, -25:] - prior).max() <= 1e-9 * np.abs(prior).max()
    # while the block over the data is not the prior
    near = O.gram(kidx, Q, D, R, m2i[:-25] if kidx == 7 else None, t2[:-25], th)
    assert np.abs(C[:-25, :-25] - near).max() > 1e-3 * np.abs(near).max()


@pytest.mark.parametrize("kidx,Q,D,R,n", FAMILIES)
def test_identity_draws_reproduce_the_covariance(kidx, Q, D, R, n):
    case = _family_case(kidx, Q, D, R, n)
    ref = restate_joint(*case)
    dev = draw(ref, np.eye(ref[0].shape[0])) - ref[0][:, None]
    np.testing.assert_allclose(dev @ dev.T, ref[2], rtol=0, atol=1e-12 * np.abs(ref[2]).max())


# ---------------------------------------------------------------------------------------------------------------------------
# the condition the GPU tests' bar rests on, for every input they use
# ---------------------------------------------------------------------------------------------------------------------------
def _assert_conditioned(fam, pt, th, tp, what):
    kidx, Q, D, R = fam
    multi = kidx == 7
    if tp[1].shape[0] == 0:
        return
    for k in (0, 3):
        C = restate_joint(kidx, Q, D, R, pt[0] if multi else None, pt[1], pt[2], th, tp[0] if multi else None, tp[1], jitter_rounds=k)[2]
        assert cond(C) <= COND_MAX, (what, k, cond(C))


@pytest.mark.parametrize("i", range(len(PC.SHAPES)), ids=[PC.shape_id(s) for s in PC.SHAPES])
def test_gpu_shapes_are_well_conditioned(i):
    pts, th, tp, _ = PC.shape_data(i)
    for p in range(len(pts)):
        _assert_conditioned(PC.SHAPES[i][:4], pts[p], th[p], tp[p], (i, p))


def test_gpu_named_cases_are_well_conditioned():
    fam, pt, th, tp, _ = PC.duplicates_case()
    _assert_conditioned(fam, pt, th, tp, "duplicates")
    for fn in (PC.jitter_case, PC.invariance_case):
        fam, pts, th, tp, _ = fn()
        for p in range(len(pts)):
            _assert_conditioned(fam, pts[p], th[p], tp[p], (fn.__name__, p))


# ---------------------------------------------------------------------------------------------------------------------------
# the checker bites
# ---------------------------------------------------------------------------------------------------------------------------
def _checked_case():
    D, Q, R = 24, 5, 8
    case = _family_case(7, Q, D, R, 300, m=130, seed=21)
    eps = np.random.default_rng(9).standard_normal((130, 7))
    return case, eps


def _f32(a):
    return np.asarray(a, np.float32)


def test_check_accepts_the_fp32_rounding_of_the_reference():
    case, eps = _checked_case()
    ref = restate_joint(*case)
    check_joint(ref, _f32(ref[1]), _f32(ref[2]), _f32(draw(ref, eps)), eps)
    check_joint(ref, _f32(ref[1]), None, _f32(draw(ref, eps)), eps)
    check_joint(ref, _f32(ref[1]), _f32(ref[2]))


def test_check_rejects_the_noise_added_twice():
    case, eps = _checked_case()
    ref = restate_joint(*case)
    wrong = ref[2] + np.diag(noise_var(7, case[2], case[7], case[8]))
    with pytest.raises(AssertionError, match="cov"):
        check_joint(ref, _f32(ref[1]), _f32(wrong))


def test_check_rejects_the_retried_noise_on_the_test_points():
    """after k = 1 retry the test points' noise is still added once, not (1 + k) times"""
    case, eps = _checked_case()
    ref = restate_joint(*case, jitter_rounds=1)
    wrong = ref[2] + np.diag(noise_var(7, case[2], case[7], case[8]))
    with pytest.raises(AssertionError, match="cov"):
        check_joint(ref, _f32(ref[1]), _f32(wrong))


def test_check_rejects_two_covariates_swapped():
    case, eps = _checked_case()
    ref = restate_joint(*case)
    m2 = case[8].copy()
    i, j = 0, int(np.argmax(m2 != m2[0]))
    m2[i], m2[j] = m2[j], m2[i]
    swapped = restate_joint(*case[:8], m2, case[9])
    with pytest.raises(AssertionError, match="cov"):
        check_joint(ref, _f32(ref[1]), _f32(swapped[2]))


def test_check_rejects_an_asymmetric_cov():
    case, eps = _checked_case()
    ref = restate_joint(*case)
    cov = _f32(ref[2]).copy()
    cov[5, 3] = np.nextafter(cov[5, 3], np.float32(np.inf))
    with pytest.raises(AssertionError, match="symmetric"):
        check_joint(ref, _f32(ref[1]), cov)


def test_check_rejects_a_diagonal_that_is_not_var():
    case, eps = _checked_case()
    ref = restate_joint(*case)
    with pytest.raises(AssertionError, match="var"):
        check_joint(ref, _f32(ref[1] * (1.0 + 1e-5)), _f32(ref[2]))


def test_check_rejects_samples_drawn_with_the_transposed_factor():
    case, eps = _checked_case()
    ref = restate_joint(*case)
    wrong = ref[0][:, None] + ref[3].T @ eps
    with pytest.raises(AssertionError, match="samples"):
        check_joint(ref, _f32(ref[1]), None, _f32(wrong), eps)

