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
from posterior_ref import restate

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
