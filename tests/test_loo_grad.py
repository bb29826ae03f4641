"""medgp_loo_grad without a GPU: the ABI surface, the long-double truth (loo_grad_truth.py) against central differences of its
own objective and against the refit definition of the LOO log pseudo-likelihood (loo_ref.py), and the conditions under which
the truth's fp64 error budget may be used to judge the device (test_loo_grad_gpu.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from medgp_amd import capi, synth
import loo_grad_truth as G
import loo_ref as LR
import nlml_truth as T
from random_patients import random_patient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_loo_grad(built_lib):
    src = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    assert re.search(r"int\s+medgp_loo_grad\s*\(", src)
    assert "tests/loo_grad_truth.py" in src
    assert hasattr(C.CDLL(built_lib), "medgp_loo_grad")
    assert "medgp_loo_grad" in capi.SYMBOLS
    lib = capi.load()
    assert lib.medgp_abi_version() >= 7
    names = [lib.medgp_profile_kernel_name(k).decode() for k in range(lib.medgp_profile_num_kernels())]
    assert {"k_loo_kinv", "k_loo_vec", "k_loo_wgrad"} <= set(names)
    # appended: the ids of the earlier kernels did not move
    assert names[15:18] == ["k_loo_diag", "k_loo_gram", "k_loo_solve"]
    blob = open(built_lib, "rb").read()
    assert b"k_loo_kinv" in blob and b"k_loo_vec" in blob and b"k_loo_wgrad" in blob


def test_null_arguments_are_argument_errors(built_lib):
    lib = capi.load()
    slots = np.zeros(1, np.int32)
    th = np.zeros(8)
    obj = np.zeros(1)
    rc = lib.medgp_loo_grad(None, 1, slots.ctypes.data_as(C.POINTER(C.c_int32)), th.ctypes.data_as(C.POINTER(C.c_double)), 0,
                            obj.ctypes.data_as(C.POINTER(C.c_double)), None, None)
    assert rc == -1   # MEDGP_ERR_ARG


def _small(kidx):
    g = T._philox(20261102, kidx)
    if kidx == 7:
        Q, D, R = 2, 3, 2
        m, t, y = random_patient(g, D, 40, "plain")
    else:
        Q, D, R = (3, 1, 0) if kidx == 8 else (1, 1, 0)
        m, t, y = None, np.sort(g.uniform(0.0, 200.0, size=40)).astype(np.float32), g.standard_normal(40).astype(np.float32)
    return (kidx, Q, D, R), m, t, y, synth.theta(4717, kidx, kidx, Q, D, R)


@pytest.mark.parametrize("kidx", [7, 8, 0], ids=["lmc", "sm", "se"])
def test_truth_gradient_is_the_derivative_of_the_truth_objective(kidx):
    """Central differences of the long-double objective at steps h and 2 h.  D(h) = g + h^2 f''' / 6 + O(h^4), so
    (D(2h) - D(h)) / 3 estimates the truncation error of D(h); rounding adds at most ~ eps |J| / h per difference (two objective
    evaluations, each good to a few eps |J|: 8 eps |J| / h allows for the conditioning of the 40-point problems).  The bound is
    twice the estimate plus that rounding term -- from the step alone, and it must itself be small against the gradient."""
    fam, m, t, y, th = _small(kidx)
    X = np.longdouble
    J, g = G.loo_grad(*fam, m, t, y, th)
    h = 1e-5
    eps = float(np.finfo(X).eps)

    def cd(i, step):
        a, b = th.copy(), th.copy()
        a[i] += step
        b[i] -= step
        return (G.loo_grad(*fam, m, t, y, a, want_grad=False)[0] - G.loo_grad(*fam, m, t, y, b, want_grad=False)[0]) / X((a[i] - b[i]))

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


@pytest.mark.parametrize("cid", [c for c in G.CASE_IDS if c != "lmc_D24_n512"])
def test_truth_objective_is_minus_the_refit_total(cid):
    c = G.case(cid)
    for p, (m, t, y) in enumerate(c["pts"]):
        J = float(G.truth_of(c, p)[0])
        tot = LR.refit(*G.fam(c), m, t, y, c["th"][p])[3]
        assert abs(J + tot) <= LR.LPD_BOUND * max(1.0, abs(tot)), (cid, p, J, tot)


def test_truth_objective_is_minus_the_refit_total_under_jitter():
    c = G.case("lmc_sizes")
    m, t, y = c["pts"][2]
    J = float(G.loo_grad(*G.fam(c), m, t, y, c["th"][2], jitter_rounds=3, want_grad=False)[0])
    tot = LR.refit(*G.fam(c), m, t, y, c["th"][2], jitter_rounds=3)[3]
    assert abs(J + tot) <= LR.LPD_BOUND * max(1.0, abs(tot))


def test_block_sum_form_equals_per_hyper_trace():
    """the form the n = 512 truth takes (loo_grad_truth.NAIVE_MAX_N) against the naive one, both in long double"""
    c = G.case("lmc_sizes")
    m, t, y = c["pts"][4]
    a = G.loo_grad(*G.fam(c), m, t, y, c["th"][4], form="naive")[1]
    b = G.loo_grad(*G.fam(c), m, t, y, c["th"][4], form="blocks")[1]
    assert T.error_pair(1.0, b.astype(np.float64), 1.0, a)[1] <= 2 * T.U64      # (b is rounded to fp64 by error_pair)
    assert float(np.max(np.abs(a - b)) / np.max(np.abs(a))) <= 1e-16


def test_budget_factor_M_and_caps():
    """The conditions of test_nlml_truth.py, for the LOO objective: two legitimate fp64 programs within M / 4 of each other on
    every case, every budget under its cap, cond(K) <= 1e4.  CPU programs only."""
    worst_sn = worst_sg = 0.0
    for cid in G.CASE_IDS:
        c = G.case(cid)
        for p, (m, t, y) in enumerate(c["pts"]):
            assert G.cond(*G.fam(c), m, t, c["th"][p]) <= G.COND_MAX, (cid, p)
            r = G.programs_of(c, p)
            sn, sg = G.spread(r["en"]), G.spread(r["eg"])
            worst_sn, worst_sg = max(worst_sn, sn), max(worst_sg, sg)
            assert G.budget(r["en"], G.M_OBJ) < G.NLML_BUDGET_CAP, (cid, p, r["en"])
            assert G.budget(r["eg"], G.M_GRAD) < G.GRAD_BUDGET_CAP, (cid, p, r["eg"])
            print(f"{cid}:{p} n {t.shape[0]} E_obj {r['en'][0]:.2g} {r['en'][1]:.2g} E_grad {r['eg'][0]:.2g} {r['eg'][1]:.2g}")

    def rule(s):   # the smallest power of two M with spread <= M / 4, not below the starting values' scale
        M = 1
        while s > M / 4:
            M *= 2
        return M

    print(f"spread between the programs: objective {worst_sn:.1f}, gradient {worst_sg:.1f} -> M_OBJ {rule(worst_sn)}, M_GRAD {rule(worst_sg)}")
    assert rule(worst_sn) <= G.M_OBJ and rule(worst_sg) <= G.M_GRAD
    assert G.M_OBJ == max(T.M_NLML, rule(worst_sn)) and G.M_GRAD == max(T.M_GRAD, rule(worst_sg))
