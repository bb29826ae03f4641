"""medgp_posterior_batch without a GPU: the ABI surface, argument errors, and the numpy restatement of parsed_predict that the
GPU tests (test_posterior_gpu.py) hold the device to, validated here against the oracle's predict."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import medgp_amd
from medgp_amd import capi, synth
from oracle import oracle as O
from posterior_ref import check_posterior, noise_var, restate, terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_posterior(built_lib):
    src = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    assert re.search(r"int\s+medgp_posterior_batch\s*\(", src)
    lib = C.CDLL(built_lib)
    assert hasattr(lib, "medgp_posterior_batch")
    assert "medgp_posterior_batch" in capi.SYMBOLS
    assert capi.load().medgp_abi_version() >= 4
    assert b"k_posterior" in open(built_lib, "rb").read() and b"k_alpha" in open(built_lib, "rb").read()


def test_null_context_is_an_argument_error(built_lib):
    lib = capi.load()
    off = np.zeros(2, np.int64)
    slots = np.zeros(1, np.int32)
    th = np.zeros(8)
    rc = lib.medgp_posterior_batch(None, 1, slots.ctypes.data_as(C.POINTER(C.c_int32)), th.ctypes.data_as(C.POINTER(C.c_double)),
                                   off.ctypes.data_as(C.POINTER(C.c_int64)), None, None, None, None, None, None)
    assert rc == -1   # MEDGP_ERR_ARG


def _offline_context(kidx=7, Q=2, D=3, R=2):
    """A Context object that never reached the library (no device here): enough for the checks done before the call."""
    ctx = medgp_amd.Context.__new__(medgp_amd.Context)
    ctx._lib, ctx._h = capi.load(), None
    ctx.kernel_index, ctx.Q, ctx.D, ctx.R, ctx.device = kidx, Q, D, R, 0
    ctx.H = O.num_hyp(kidx, Q, D, R)
    return ctx


@pytest.mark.parametrize("case", ["theta", "npatients", "nmeta", "ragged", "meta_missing"])
def test_posterior_rejects_mismatched_inputs(built_lib, case):
    ctx = _offline_context()
    th = np.zeros((2, ctx.H))
    m2 = [np.zeros(3, np.int32), np.zeros(1, np.int32)]
    t2 = [np.zeros(3, np.float32), np.zeros(1, np.float32)]
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
    with pytest.raises(ValueError):
        ctx.posterior([0, 1], th, m2, t2)


@pytest.mark.parametrize("kidx,Q,D,R,n", [(7, 3, 3, 2, 70), (7, 5, 24, 8, 300), (8, 3, 1, 0, 50), (0, 1, 1, 0, 40)])
def test_restatement_matches_oracle_predict(kidx, Q, D, R, n):
    meta, t, y = synth.patient(11, 0, D, n, interleave=True)
    th = synth.theta(11, 0, kidx, Q, D, R)
    g = np.random.default_rng(3)
    m2 = g.integers(0, D, size=40).astype(np.int32)
    t2 = g.uniform(-5.0, float(t.max()) + 5.0, size=40).astype(np.float32)
    mi, m2i = (meta, m2) if kidx == 7 else (None, None)
    mean, var, parts = restate(kidx, Q, D, R, mi, t, y, th, m2i, t2)
    ref = O.fit_predict(kidx, Q, D, R, mi, t, y, th, m2i, t2)
    assert ref["status"] == 0
    sc = np.abs(ref["mean"]).max()
    np.testing.assert_allclose(mean, ref["mean"], rtol=1e-8, atol=1e-9 * sc)
    np.testing.assert_allclose(var, ref["var"], rtol=1e-8, atol=1e-9 * np.abs(ref["var"]).max())
    assert parts.shape == (40, D if kidx == 7 else 1)
    np.testing.assert_allclose(parts.sum(axis=1), mean, rtol=1e-9, atol=1e-10 * sc)


def _scaled_noise(kidx, D, th, k):
    """theta whose noise variance is (1 + k) x the original (as _theta_noise in test_parity2_gpu.py)"""
    th2 = np.array(th, np.float64)
    th2[:O.num_lik(kidx, D)] += 0.5 * np.log1p(k)
    return th2


@pytest.mark.parametrize("kidx,Q,D,R,n,k", [(7, 3, 3, 2, 70, 1), (7, 5, 24, 8, 150, 3), (7, 2, 4, 2, 130, 10), (0, 1, 1, 0, 40, 2),
                                           (8, 3, 1, 0, 50, 10)])
def test_restatement_with_jitter_rounds_matches_oracle_at_scaled_noise(kidx, Q, D, R, n, k):
    """k retries factor K + k diag(sigma^2) = the Gram at (1 + k) sigma^2; the test points' noise is added once, so the oracle
    at the scaled noise has the same mean and a var larger by k sigma^2_{meta2}."""
    meta, t, y = synth.patient(12, k, D, n, interleave=True)
    th = synth.theta(12, k, kidx, Q, D, R)
    g = np.random.default_rng(4)
    m2 = g.integers(0, D, size=30).astype(np.int32)
    t2 = g.uniform(-5.0, float(t.max()) + 5.0, size=30).astype(np.float32)
    mi, m2i = (meta, m2) if kidx == 7 else (None, None)
    mean, var, parts = restate(kidx, Q, D, R, mi, t, y, th, m2i, t2, jitter_rounds=k)
    ref = O.fit_predict(kidx, Q, D, R, mi, t, y, _scaled_noise(kidx, D, th, k), m2i, t2)
    assert ref["status"] == 0
    sig2 = noise_var(kidx, D, th, m2 if kidx == 7 else np.zeros(30, np.int32))
    np.testing.assert_allclose(mean, ref["mean"], rtol=1e-8, atol=1e-9 * np.abs(ref["mean"]).max())
    np.testing.assert_allclose(var, ref["var"] - k * sig2, rtol=1e-8, atol=1e-9 * np.abs(ref["var"]).max())
    np.testing.assert_allclose(parts.sum(axis=1), mean, rtol=1e-9, atol=1e-10 * np.abs(mean).max())
    # and it is not the unretried posterior
    m0, v0, _ = restate(kidx, Q, D, R, mi, t, y, th, m2i, t2)
    assert np.abs(v0 - var).max() > 1e-6 * np.abs(v0).max()


@pytest.mark.parametrize("D,n,missing", [(3, 1, False), (3, 2, False), (64, 40, False), (64, 300, False), (6, 90, True)])
def test_restatement_matches_oracle_at_edges(D, n, missing):
    """n = 1 and n = 2 (the predict path has no n > 2 guard), D = 64, and covariates without a training observation, whose
    parts are exactly 0."""
    Q, R = 3, min(D, 4)
    g = np.random.default_rng(100 + n)
    outs = np.arange(0, D, 2) if missing else np.arange(D)
    meta = np.sort(g.choice(outs, size=n)).astype(np.int32)
    t = g.uniform(0.0, 200.0, size=n).astype(np.float32)
    for d in outs:
        t[meta == d] = np.sort(t[meta == d])
    y = g.standard_normal(n).astype(np.float32)
    th = synth.theta(13, n, 7, Q, D, R)
    m2 = g.integers(0, D, size=50).astype(np.int32)
    t2 = g.uniform(-5.0, 205.0, size=50).astype(np.float32)
    mean, var, parts = restate(7, Q, D, R, meta, t, y, th, m2, t2)
    ref = O.fit_predict(7, Q, D, R, meta, t, y, th, m2, t2)
    assert ref["status"] == 0
    np.testing.assert_allclose(mean, ref["mean"], rtol=1e-8, atol=1e-9 * np.abs(ref["mean"]).max())
    np.testing.assert_allclose(var, ref["var"], rtol=1e-8, atol=1e-9 * np.abs(ref["var"]).max())
    absent = np.setdiff1d(np.arange(D), meta)
    assert np.all(parts[:, absent] == 0.0)
    if missing:
        assert absent.size >= D // 2
    np.testing.assert_allclose(parts.sum(axis=1), mean, rtol=1e-9, atol=1e-10 * np.abs(mean).max())


def _checked_case():
    """the shape of the issue's sensitivity measurement: D = 24, Q = 5, R = 8, n = 300, test points over the data and 3 h beyond"""
    D, Q, R = 24, 5, 8
    meta, t, y = synth.patient(21, 0, D, 300, interleave=True)
    th = synth.theta(21, 0, 7, Q, D, R)
    g = np.random.default_rng(100)
    m2 = g.integers(0, D, size=130).astype(np.int32)
    t2 = g.uniform(float(t.min()) - 3.0, float(t.max()) + 3.0, size=130).astype(np.float32)
    return (7, Q, D, R, meta, t, y, th, m2, t2)


def _f32(a):
    return np.asarray(a, np.float32)


def test_check_accepts_the_fp32_rounding_of_the_reference():
    kidx, Q, D, R, meta, t, y, th, m2, t2 = case = _checked_case()
    ref = restate(*case)
    check_posterior(kidx, D, th, m2, ref, _f32(ref[0]), _f32(ref[1]), _f32(ref[2]))


def test_check_rejects_var_at_test_times_one_ulp_off():
    """every test time moved by one float32 ulp: var alone (mean and parts exact) must fail the check"""
    kidx, Q, D, R, meta, t, y, th, m2, t2 = case = _checked_case()
    ref = restate(*case)
    t2s = np.nextafter(t2, np.float32(np.inf)).astype(np.float32)
    shifted = restate(kidx, Q, D, R, meta, t, y, th, m2, t2s)
    with pytest.raises(AssertionError, match="var"):
        check_posterior(kidx, D, th, m2, ref, _f32(ref[0]), _f32(shifted[1]), _f32(ref[2]))


def test_check_rejects_var_with_the_retried_noise():
    """var formed with (1 + k) sigma^2 after k = 1 retry instead of adding the noise once"""
    kidx, Q, D, R, meta, t, y, th, m2, t2 = case = _checked_case()
    ref = restate(*case, jitter_rounds=1)
    wrong = ref[1] + noise_var(kidx, D, th, m2)
    with pytest.raises(AssertionError, match="var"):
        check_posterior(kidx, D, th, m2, ref, _f32(ref[0]), _f32(wrong), _f32(ref[2]))


@pytest.mark.parametrize("row", [63, 64])
def test_check_rejects_a_part_moved_across_a_panel_boundary(row):
    """the contribution K*[row, :] alpha[row] of the last row of a 64-row panel / the first row of the next one booked to the
    neighbouring covariate: the mean (and the sum of the parts) is unchanged, the parts must fail the check"""
    kidx, Q, D, R, meta, t, y, th, m2, t2 = case = _checked_case()
    ref = restate(*case)
    Ks, alpha, *_ = terms(*case)
    moved = ref[2].copy()
    d = int(meta[row])
    moved[:, d] -= Ks[row] * alpha[row]
    moved[:, (d + 1) % D] += Ks[row] * alpha[row]
    assert np.allclose(moved.sum(axis=1), ref[0], rtol=1e-12, atol=1e-12 * np.abs(ref[0]).max())
    with pytest.raises(AssertionError, match="parts"):
        check_posterior(kidx, D, th, m2, ref, _f32(ref[0]), _f32(ref[1]), _f32(moved))
