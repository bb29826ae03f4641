"""medgp_forecast_grad without a GPU: the ABI surface, the long-double truth (forecast_grad_truth.py) against central differences
of its own objective, against the refit definition of medgp_forecast_batch's lpd (forecast_ref.py) and against nlml_truth in the
chain-rule case, the prefix builder, the host table program under the sanitizers, and the conditions under which the truth's fp64
error budget may be used to judge the device (test_forecast_grad_gpu.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from medgp_amd import capi, forecast, synth
import forecast_grad_truth as F
import forecast_ref as FR
import nlml_truth as T
from random_patients import random_patient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medgp_amd", "csrc")


def test_header_declares_and_library_exports_forecast_grad(built_lib):
    src = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    assert re.search(r"int\s+medgp_forecast_grad\s*\(", src)
    assert "tests/forecast_grad_truth.py" in src and "2^14 h" in src.split("medgp_forecast_grad(")[0][-3000:]
    assert hasattr(C.CDLL(built_lib), "medgp_forecast_grad")
    assert "medgp_forecast_grad" in capi.SYMBOLS
    lib = capi.load()
    assert lib.medgp_abi_version() >= 14
    names = [lib.medgp_profile_kernel_name(k).decode() for k in range(lib.medgp_profile_num_kernels_all())]
    # appended behind the frozen table: neither its length nor the ids of the earlier kernels moved
    assert lib.medgp_profile_num_kernels() == 23 and names[19:23] == ["k_loo_vec", "k_loo_wgrad", "k_trend", "k_forecast"]
    assert names[23:] == ["k_fc_vec", "k_fc_t", "k_fc_scan", "k_fc_qm", "k_fc_tables", "k_fc_wgrad"]
    blob = open(built_lib, "rb").read()
    assert b"k_fc_vec" in blob and b"k_fc_t" in blob and b"k_fc_wgrad" in blob


def test_null_arguments_are_argument_errors(built_lib):
    lib = capi.load()
    slots = np.zeros(1, np.int32)
    th = np.zeros(8)
    obj = np.zeros(1)
    rc = lib.medgp_forecast_grad(None, 1, slots.ctypes.data_as(C.POINTER(C.c_int32)), th.ctypes.data_as(C.POINTER(C.c_double)), None, None, 0,
                                 obj.ctypes.data_as(C.POINTER(C.c_double)), None, None)
    assert rc == -1   # MEDGP_ERR_ARG


def test_table_program_against_brute_force_under_sanitizers():
    subprocess.check_call(["make", "-s", "-C", CSRC, "forecast_grad_tables_test"])
    out = subprocess.run([os.path.join(CSRC, "forecast_grad_tables_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "forecast_grad_tables ok" in out.stdout


def test_training_prefix():
    t = np.array([0.0, 1.0, 1.0, 1.0, 2.5, 7.0, 7.0, 9.0], np.float32)
    # strictly earlier: tied observations never condition on each other
    assert forecast.training_prefix(t, 0.0).tolist() == [0, 1, 1, 1, 4, 5, 5, 7]
    assert forecast.training_prefix(t, 6.0).tolist() == [0, 0, 0, 0, 0, 1, 1, 5]
    assert forecast.training_prefix(t, 6.0, min_history=1).tolist() == [-1, -1, -1, -1, -1, 1, 1, 5]
    assert forecast.training_prefix(t, 0.0, min_history=5).tolist() == [-1, -1, -1, -1, -1, 5, 5, 7]
    p = forecast.training_prefix(t, 1e6)
    assert p.dtype == np.int32 and p.tolist() == [0] * 8
    assert forecast.training_prefix(np.zeros(0, np.float32), 1.0).shape == (0,)
    # the table is rolling_origin's prefix for that horizon, and a valid argument of the call
    assert np.array_equal(forecast.training_prefix(t, 6.0), forecast.rolling_origin(None, t, t, [6.0])[3])
    assert np.all(forecast.training_prefix(t, 0.0) <= np.arange(8))
    with pytest.raises(ValueError):
        forecast.training_prefix(t[::-1], 0.0)
    with pytest.raises(ValueError):
        forecast.training_prefix(t, -1.0)
    with pytest.raises(ValueError):
        forecast.training_prefix(t, 1.0, min_history=-1)


def _small(kidx):
    g = T._philox(20261202, kidx)
    if kidx == 7:
        Q, D, R = 2, 3, 2
        m, t, y = random_patient(g, D, 40, "plain")
        o = np.argsort(t, kind="stable")
        m, t, y = m[o], t[o], y[o]
    else:
        Q, D, R = (3, 1, 0) if kidx == 8 else (1, 1, 0)
        m, t, y = None, np.sort(g.uniform(0.0, 200.0, size=40)).astype(np.float32), g.standard_normal(40).astype(np.float32)
    return (kidx, Q, D, R), m, t, y, synth.theta(4718, kidx, kidx, Q, D, R)


@pytest.mark.parametrize("kidx", [7, 8, 0], ids=["lmc", "sm", "se"])
def test_truth_gradient_is_the_derivative_of_the_truth_objective(kidx):
    """Central differences of the long-double refit objective at steps h and 2 h, with the Richardson bound of test_loo_grad.py:
    D(h) = g + h^2 f''' / 6 + O(h^4), so (D(2h) - D(h)) / 3 estimates the truncation error of D(h); rounding adds at most
    8 eps |J| / h.  The prefix table (6 h, with unscored observations among the first) stays fixed while theta moves."""
    fam, m, t, y, th = _small(kidx)
    X = np.longdouble
    pf = forecast.training_prefix(t, 6.0, min_history=2)
    assert np.any(pf < 0) and np.any(pf > 0) and np.any(pf[pf >= 0] < np.arange(40)[pf >= 0])
    J, g = F.forecast_grad(*fam, m, t, y, th, pf)
    h = 1e-5
    eps = float(np.finfo(X).eps)

    def cd(i, step):
        a, b = th.copy(), th.copy()
        a[i] += step
        b[i] -= step
        return (F.forecast_grad(*fam, m, t, y, a, pf, want_grad=False)[0] - F.forecast_grad(*fam, m, t, y, b, pf, want_grad=False)[0]) / X((a[i] - b[i]))

    gs = float(np.abs(g).max())
    worst = 0.0
    for i in range(th.shape[0]):
        d1, d2 = cd(i, h), cd(i, 2 * h)
        tol = 2 * float(abs(d2 - d1)) / 3 + 8 * eps * float(abs(J)) / h
        assert tol <= 1e-6 * gs, (i, tol, gs)          # the check has teeth
        err = float(abs(d1 - g[i]))
        worst = max(worst, err / gs)
        assert err <= tol, (i, float(g[i]), float(d1), err, tol)
    print(f"central differences, kernel {kidx}: worst |D(h) - g| / max|g| = {worst:.2g}")


@pytest.mark.parametrize("cid", F.CASE_IDS)
def test_truth_objective_is_minus_the_sum_of_forecast_lpd(cid):
    """J and every lpd_i against forecast_ref.refit with a test point placed at the observation, on the same prefixes"""
    c = F.case(cid)
    for p, (m, t, y) in enumerate(c["pts"]):
        for h in F.HORIZONS:
            pf = F.prefix_of(c, p, h)
            J, _, lpd, _ = F.forecast_grad(*F.fam(c), m, t, y, c["th"][p], pf, want_grad=False, want_parts=True)
            ref = FR.refit(*F.fam(c), m, t, y, c["th"][p], m, t, pf, y)[2]
            assert FR.lpd_error(lpd.astype(np.float64), ref) <= FR.lpd_bound(), (cid, p, h)
            assert abs(float(J) + ref.sum()) <= FR.lpd_bound() * np.sum(np.maximum(1.0, np.abs(ref))), (cid, p, h)


@pytest.mark.parametrize("cid", ["lmc_sizes", "sm_Q4", "se"])
def test_full_history_is_the_chain_rule_of_the_likelihood(cid):
    """prefix[i] = i, all scored: J is nlml_truth's nlml (no prior) and the gradient its gradient, in long double"""
    c = F.case(cid)
    for p, (m, t, y) in enumerate(c["pts"]):
        n = t.shape[0]
        if n <= 2 or n > 130:
            continue
        J, g = F.forecast_grad(*F.fam(c), m, t, y, c["th"][p], None)
        _, nl, gn = T.nlml_grad(*F.fam(c), m, t, y, c["th"][p])
        assert abs(J - nl) <= 1e-15 * abs(nl), (cid, p, float(J), float(nl))
        assert float(np.max(np.abs(g - gn)) / np.max(np.abs(gn))) <= 1e-13, (cid, p)


def test_empty_history_gives_a_diagonal_w():
    c = F.case("lmc_sizes")
    m, t, y = c["pts"][2]
    n = t.shape[0]
    off = ~np.eye(n, dtype=bool)
    W = F.forecast_grad(*F.fam(c), m, t, y, c["th"][2], np.zeros(n, np.int64), want_parts=True)[3]
    assert np.all(W[off] == 0) and np.all(np.diagonal(W) != 0)
    # the one-factor program forms u_i = U L[i, 0:i+1]^T = e_i by a product: diagonal up to its rounding
    W1 = F.one_factor(*F.fam(c), m, t, y, c["th"][2], np.zeros(n, np.int64), want_parts=True)[3]
    assert np.max(np.abs(W1[off])) <= 1e-12 * np.max(np.abs(np.diagonal(W1)))
    assert np.max(np.abs(np.diagonal(W1) - np.diagonal(W).astype(np.float64))) <= 1e-12 * np.max(np.abs(np.diagonal(W1)))
    # nothing scored: J = 0, W = 0
    J, g, lpd, W = F.forecast_grad(*F.fam(c), m, t, y, c["th"][2], np.full(n, -1), want_parts=True)
    assert J == 0 and np.all(g == 0) and np.all(W == 0) and np.all(lpd == 0)


def test_one_factor_program_is_the_refit_program():
    """the identities the device uses (program (c)) against the refit (program (b)), element by element of lpd and W"""
    c = F.case("lmc_sizes")
    m, t, y = c["pts"][4]
    pf = forecast.training_prefix(t, 6.0, min_history=1)
    assert np.any(pf < 0)
    for jit in (0, 2):
        a = F.forecast_grad(*F.fam(c), m, t, y, c["th"][4], pf, np.float64, jit, want_parts=True)
        b = F.one_factor(*F.fam(c), m, t, y, c["th"][4], pf, jit, want_parts=True)
        assert abs(a[0] - b[0]) <= 1e-12 * abs(a[0])
        assert np.max(np.abs(a[2] - b[2])) <= 1e-11 * np.max(np.abs(a[2]))
        assert np.max(np.abs(a[3] - b[3])) <= 1e-9 * np.max(np.abs(a[3]))


def test_budget_factor_M_and_caps():
    """The conditions of test_loo_grad.py, for the forecast objective: the two fp64 programs within M / 4 of each other on every
    (patient, horizon) pair, every budget under its cap, cond(K) <= 1e4.  CPU programs only."""
    worst_sn = worst_sg = 0.0
    pairs = F.all_pairs()
    assert len(pairs) == 22
    for cid, p, h in pairs:
        c = F.case(cid)
        m, t, y = c["pts"][p]
        assert t.shape[0] < 2 or np.all(np.diff(t) >= 0)
        assert F.cond(*F.fam(c), m, t, c["th"][p]) <= F.COND_MAX, (cid, p)
        r = F.programs_of(c, p, F.prefix_of(c, p, h))
        sn, sg = F.spread(r["en"]), F.spread(r["eg"])
        worst_sn, worst_sg = max(worst_sn, sn), max(worst_sg, sg)
        assert F.budget(r["en"], F.M_OBJ) < F.NLML_BUDGET_CAP, (cid, p, h, r["en"])
        assert F.budget(r["eg"], F.M_GRAD) < F.GRAD_BUDGET_CAP, (cid, p, h, r["eg"])
        print(f"{cid}:{p} h {h:g} n {t.shape[0]} E_obj {r['en'][0]:.2g} {r['en'][1]:.2g} E_grad {r['eg'][0]:.2g} {r['eg'][1]:.2g}")
    print(f"spread between the programs: objective {worst_sn:.1f}, gradient {worst_sg:.1f}")
    assert worst_sn <= F.M_OBJ / 4 and worst_sg <= F.M_GRAD / 4
    assert F.M_OBJ == 256 and F.M_GRAD == 128 and F.COND_MAX == 1e4
    # the interleaving the call exists for: the time-sorted multi-output patients are not grouped by output
    c = F.case("lmc_sizes")
    assert all(np.any(np.diff(c["pts"][p][0]) < 0) for p in range(2, 7))
