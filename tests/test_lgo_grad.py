"""medgp_lgo_grad without a GPU: the ABI surface, the long-double truth (lgo_grad_truth.py) against the refit definition of the
leave-group-out log pseudo-likelihood (loo_ref.py), against central differences of its own objective and against its two exact
special cases (all singletons = the LOO truth, one group of everything = the nlml truth), the conditions under which the truth's fp64
error budget may be used to judge the device (test_lgo_grad_gpu.py), the group builders of medgp_amd/crossval.py, and the host
table extension's own test program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from medgp_amd import capi, crossval, synth
import lgo_grad_truth as G
import loo_grad_truth as LG
import loo_ref as LR
import nlml_truth as T
from random_patients import random_patient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medgp_amd", "csrc")


def test_header_declares_and_library_exports_lgo_grad(built_lib):
    src = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    assert re.search(r"int\s+medgp_lgo_grad\s*\(", src)
    assert "tests/lgo_grad_truth.py" in src
    assert hasattr(C.CDLL(built_lib), "medgp_lgo_grad")
    assert "medgp_lgo_grad" in capi.SYMBOLS
    lib = capi.load()
    assert lib.medgp_abi_version() >= 15
    assert lib.medgp_profile_num_kernels() == 23          # the frozen table
    assert lib.medgp_profile_num_kernels_all() == 29      # ... and the one behind it, which test_forecast_grad.py compares as a whole
    names = [lib.medgp_profile_kernel_name(k).decode() for k in range(lib.medgp_profile_num_kernels_ext())]
    assert {"k_lgo_vec", "k_lgo_inv", "k_lgo_s", "k_lgo_t", "k_lgo_wgrad"} <= set(names[29:])      # appended behind both
    assert names[23:29] == ["k_fc_vec", "k_fc_t", "k_fc_scan", "k_fc_qm", "k_fc_tables", "k_fc_wgrad"]
    blob = open(built_lib, "rb").read()
    assert b"k_lgo_s" in blob and b"k_lgo_t" in blob and b"k_lgo_wgrad" in blob
    assert hasattr(capi.Context, "lgo_grad")


def test_null_arguments_are_argument_errors(built_lib):
    lib = capi.load()
    slots = np.zeros(1, np.int32)
    th = np.zeros(8)
    obj = np.zeros(1)
    rc = lib.medgp_lgo_grad(None, 1, slots.ctypes.data_as(C.POINTER(C.c_int32)), th.ctypes.data_as(C.POINTER(C.c_double)), None, None, 0,
                            obj.ctypes.data_as(C.POINTER(C.c_double)), None, None, None)
    assert rc == -1   # MEDGP_ERR_ARG


def test_host_table_extension_under_sanitizers():
    """build_lgo_tables (inference_tables.h) against restatements: a stand-alone program built with the host compiler under
    -fsanitize=address,undefined and started as an ordinary child process"""
    subprocess.check_call(["make", "-s", "-C", CSRC, "lgo_tables_test"])
    out = subprocess.run([os.path.join(CSRC, "lgo_tables_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "lgo_tables ok" in out.stdout


SMALL_N = 24


def _small(kidx):
    """24 observations, not test_loo_grad.py's 40: the rounding term of the check below (8 eps |J| / h) was sized on the LOO objective,
    one factorisation; the LGO objective factors K and then every M_g, and at 40 points its long-double rounding noise in D(h)
    (measured by halving h below the truncation: +-2.3e-11 on the SM case) exceeds that term (1.8e-11).  Noise grows faster with n than
    |J| does, so the smaller patient keeps the issue's bound as it stands."""
    g = T._philox(20261210, kidx)
    n = SMALL_N
    if kidx == 7:
        Q, D, R = 2, 3, 2
        m, t, y = random_patient(g, D, n, "plain")
    else:
        Q, D, R = (3, 1, 0) if kidx == 8 else (1, 1, 0)
        m, t, y = None, np.sort(g.uniform(0.0, 200.0, size=n)).astype(np.float32), g.standard_normal(n).astype(np.float32)
    ids = g.integers(-1, 5, size=n)          # five groups of about four members, about four observations never held out
    assert (ids == -1).sum() >= 2 and np.bincount(ids + 1).max() >= 3
    return (kidx, Q, D, R), m, t, y, synth.theta(4718, kidx, kidx, Q, D, R), ids.astype(np.int32), 5


@pytest.mark.parametrize("kidx", [7, 8, 0], ids=["lmc", "sm", "se"])
def test_truth_gradient_is_the_derivative_of_the_truth_objective(kidx):
    """test_loo_grad.py's check: central differences of the long-double objective at steps h and 2 h.  D(h) = g + h^2 f''' / 6 +
    O(h^4), so (D(2h) - D(h)) / 3 estimates the truncation error of D(h); rounding adds at most ~ eps |J| / h per difference (8 eps
    |J| / h allows for the conditioning of the 40-point problems).  The bound is twice the estimate plus that rounding term -- from the
    step alone, and it must itself be small against the gradient.  Groups: random ids in [-1, 5), id -1 included."""
    fam, m, t, y, th, grp, ng = _small(kidx)
    X = np.longdouble
    J, g = G.lgo_grad(*fam, m, t, y, th, grp, ng)
    h = 1e-5
    eps = float(np.finfo(X).eps)

    def cd(i, step):
        a, b = th.copy(), th.copy()
        a[i] += step
        b[i] -= step
        return (G.lgo_grad(*fam, m, t, y, a, grp, ng, want_grad=False)[0] - G.lgo_grad(*fam, m, t, y, b, grp, ng, want_grad=False)[0]) / X((a[i] - b[i]))

    gs = float(np.abs(g).max())
    worst = used = 0.0
    for i in range(th.shape[0]):
        d1, d2 = cd(i, h), cd(i, 2 * h)
        tol = 2 * float(abs(d2 - d1)) / 3 + 8 * eps * float(abs(J)) / h
        assert tol <= 1e-6 * gs, (i, tol, gs)          # the check has teeth
        err = float(abs(d1 - g[i]))
        worst, used = max(worst, err / gs), max(used, err / tol)
        assert err <= tol, (i, float(g[i]), float(d1), err, tol)
    print(f"central differences, kernel {kidx}: worst |D(h) - g| / max|g| = {worst:.2g}, worst share of the bound {used:.2f}")


_CPU_KEYS = G.keys()


def test_truth_objective_is_minus_the_refit_total():
    for cid, p, scheme in _CPU_KEYS:
        c = G.case(cid)
        m, t, y = c["pts"][p]
        grp, ng = G.groups_of(c, p, scheme)
        J = float(G.truth_of(c, p, scheme)[0])
        tot = LR.refit(*G.fam(c), m, t, y, c["th"][p], grp, ng)[3]
        assert abs(J + tot) <= 1e-12 * max(1.0, abs(J)), (cid, p, scheme, J, tot)


def test_truth_objective_is_minus_the_refit_total_under_jitter():
    c = G.case("lmc_sizes")
    m, t, y = c["pts"][2]
    grp, ng = G.groups_of(c, 2, "rand")
    J = float(G.lgo_grad(*G.fam(c), m, t, y, c["th"][2], grp, ng, jitter_rounds=3, want_grad=False)[0])
    tot = LR.refit(*G.fam(c), m, t, y, c["th"][2], grp, ng, jitter_rounds=3)[3]
    assert abs(J + tot) <= 1e-12 * max(1.0, abs(J))


def _rel(a, b):
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("cid,p", [("lmc_sizes", 2), ("lmc_sizes", 4), ("sm_Q4", 0), ("se", 0)])
def test_all_singletons_is_the_loo_truth(cid, p):
    c = G.case(cid)
    m, t, y = c["pts"][p]
    n = t.shape[0]
    J, g = G.lgo_grad(*G.fam(c), m, t, y, c["th"][p], np.arange(n), n)
    J2, g2 = LG.loo_grad(*G.fam(c), m, t, y, c["th"][p])
    assert _rel(J, J2) <= 1e-17 and _rel(g, g2) <= 1e-17, (_rel(J, J2), _rel(g, g2))


@pytest.mark.parametrize("cid,p", [("lmc_sizes", 2), ("lmc_sizes", 4), ("sm_Q4", 0), ("se", 0)])
def test_one_group_of_everything_is_the_nlml_truth(cid, p):
    c = G.case(cid)
    m, t, y = c["pts"][p]
    J, g = G.truth_of(c, p, "all")
    _, J2, g2 = T.nlml_grad(*G.fam(c), m, t, y, c["th"][p])
    assert _rel(J, J2) <= 1e-17 and _rel(g, g2) <= 1e-17, (_rel(J, J2), _rel(g, g2))


def test_block_sum_form_equals_per_hyper_trace():
    """the form the n = 512 truth takes (NAIVE_MAX_N) against the naive one, both in long double"""
    c = G.case("lmc_sizes")
    m, t, y = c["pts"][4]
    grp, ng = G.groups_of(c, 4, "rand")
    a = G.lgo_grad(*G.fam(c), m, t, y, c["th"][4], grp, ng, form="naive")[1]
    b = G.lgo_grad(*G.fam(c), m, t, y, c["th"][4], grp, ng, form="blocks")[1]
    assert float(np.max(np.abs(a - b)) / np.max(np.abs(a))) <= 1e-16


def test_budget_factor_M_and_caps():
    """The conditions of test_loo_grad.py, for the LGO objective: two legitimate fp64 programs within M / 4 of each other on every
    case and scheme the GPU tests use, every budget under its cap, cond(K) <= 1e4.  CPU programs only."""
    worst_sn = worst_sg = 0.0
    conds = set()
    extra = [("lmc_sizes", p, "all") for p in (2, 4, 5, 6)] + [("lmc_sizes", 4, "hold")]
    for cid, p, scheme in G.keys() + extra:
        c = G.case(cid)
        m, t, y = c["pts"][p]
        if (cid, p) not in conds:
            assert G.cond(*G.fam(c), m, t, c["th"][p]) <= G.COND_MAX, (cid, p)
            conds.add((cid, p))
        r = G.programs_of(c, p, scheme)
        sn, sg = G.spread(r["en"]), G.spread(r["eg"])
        worst_sn, worst_sg = max(worst_sn, sn), max(worst_sg, sg)
        assert G.budget(r["en"], G.M_OBJ) < G.NLML_BUDGET_CAP, (cid, p, scheme, r["en"])
        assert G.budget(r["eg"], G.M_GRAD) < G.GRAD_BUDGET_CAP, (cid, p, scheme, r["eg"])
        print(f"{cid}:{p}:{scheme} n {t.shape[0]} E_obj {r['en'][0]:.2g} {r['en'][1]:.2g} E_grad {r['eg'][0]:.2g} {r['eg'][1]:.2g}")
    for fails in (1, 3):                       # the jitter cases of the GPU test
        for p in (2, 4, 5):
            r = G.programs_of(G.case("lmc_sizes"), p, "cov", fails)
            worst_sn, worst_sg = max(worst_sn, G.spread(r["en"])), max(worst_sg, G.spread(r["eg"]))
            assert G.budget(r["en"], G.M_OBJ) < G.NLML_BUDGET_CAP and G.budget(r["eg"], G.M_GRAD) < G.GRAD_BUDGET_CAP, (p, fails)

    def rule(s):   # the smallest power of two M with spread <= M / 4
        M = 1
        while s > M / 4:
            M *= 2
        return M

    print(f"spread between the programs: objective {worst_sn:.1f}, gradient {worst_sg:.1f} -> M_OBJ {rule(worst_sn)}, M_GRAD {rule(worst_sg)}")
    assert worst_sn <= G.M_OBJ / 4 and worst_sg <= G.M_GRAD / 4
    assert G.M_OBJ == max(LG.M_OBJ, rule(worst_sn)) and G.M_GRAD == max(LG.M_GRAD, rule(worst_sg))


# ---- medgp_amd/crossval.py ----------------------------------------------------------------------------------------------------------

def _check_table(grp, ng, n):
    assert grp.dtype == np.int32 and grp.shape == (n,) and isinstance(ng, int)
    assert n == 0 or (grp.min() >= -1 and grp.max() < ng)          # every observation in exactly one group or -1: one id each


def test_crossval_builders():
    g = T._philox(20261211, 0)
    m, t, y = random_patient(g, 5, 97, "shuffled")
    n = m.shape[0]
    grp, ng = crossval.by_covariate(m)
    _check_table(grp, ng, n)
    assert ng == int(m.max()) + 1 and np.array_equal(grp, m)
    assert crossval.by_covariate(m, 24)[1] == 24
    with pytest.raises(ValueError):
        crossval.by_covariate(m, int(m.max()))
    grp, ng = crossval.by_window(t, 24.0)
    _check_table(grp, ng, n)
    o = np.argsort(t, kind="stable")
    assert np.all(np.diff(grp[o]) >= 0) and grp[o][0] == 0 and grp.min() >= 0            # monotone in t, everything scored
    assert ng == int(np.floor((t.max() - t.min()) / 24.0)) + 1
    for w in range(ng):
        tt = t[grp == w].astype(np.float64) - float(t.min())
        assert tt.size == 0 or (tt.min() >= 24.0 * w and tt.max() < 24.0 * (w + 1))
    grp2, ng2 = crossval.by_covariate_window(m, t, 24.0, 5)
    _check_table(grp2, ng2, n)
    assert ng2 == 5 * ng and np.array_equal(grp2 % 5, m) and np.array_equal(grp2 // 5, grp)
    for k in (1, 2, 5, 7, 97, 120):
        f, nk = crossval.k_fold(n, k, 11)
        _check_table(f, nk, n)
        cnt = np.bincount(f, minlength=k)
        assert nk == k and f.min() >= 0 and cnt.max() - cnt.min() <= 1 and cnt.sum() == n
        assert np.array_equal(f, crossval.k_fold(n, k, 11)[0])                                # seeded
    assert not np.array_equal(crossval.k_fold(n, 5, 11)[0], crossval.k_fold(n, 5, 12)[0])
    h, nh = crossval.hold_out(n, [3, 50, 96])
    _check_table(h, nh, n)
    assert nh == 1 and np.array_equal(np.flatnonzero(h == 0), [3, 50, 96]) and (h == -1).sum() == n - 3
    with pytest.raises(ValueError):
        crossval.hold_out(n, [n])
    for fn in (lambda: crossval.by_window(np.zeros(0), 24.0), lambda: crossval.by_covariate(np.zeros(0, np.int32)), lambda: crossval.k_fold(0, 3)):
        e, ne = fn()
        assert e.shape == (0,) and e.dtype == np.int32
    with pytest.raises(ValueError):
        crossval.by_window(t, 0.0)
