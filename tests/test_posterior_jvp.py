"""medgp_posterior_jvp_batch without a GPU: the long-double truth (posterior_jvp_truth.py) against Richardson differences of the
long-double posterior, the scale identity, the closed form of a noise direction, the conditions under which the truth's fp64 error
budget may be used to judge the device (test_posterior_jvp_gpu.py), medgp_amd/sensitivity.py on analytic inputs, the ABI surface, and
the host geometry's own test program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from medgp_amd import capi, curvature, information, sensitivity
import loo_grad_truth as LG
import nlml_truth as T
import posterior_jvp_truth as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medgp_amd", "csrc")
X = np.longdouble
EPS = float(np.finfo(X).eps)

# the patients with n <= 130 that have test points (from the specs alone: nothing is built at collection)
SMALL = [(s[0], p) for s in LG._SPECS for p, (n, _) in enumerate(s[5]) if n <= 130 and PT.CASE_POINTS[s[0]][p] > 0]


def _inputs(cid, p, count=None):
    c = PT.case(cid)
    m, t, y = c["pts"][p]
    m2, t2 = PT.points(c, p, count)
    return c, PT.fam(c), m, t, y, c["th"][p], m2, t2


def test_the_cases_meet_every_tile_edge_and_a_covariate_without_observations():
    counts = sorted({PT.points(PT.case(cid), p)[1].shape[0] for cid, p in PT.patients()})
    assert counts == sorted(PT.POINT_COUNTS)
    assert sorted(PT.case("lmc_sizes")["pts"][p][1].shape[0] for p in range(7)) == [1, 3, 63, 64, 65, 130, 200]
    c = PT.case("lmc_D24_missing")
    m2, t2 = PT.points(c, 0)
    assert set(m2.tolist()) - set(np.asarray(c["pts"][0][0]).tolist())          # test points of a covariate that has no observation
    t = c["pts"][0][1]
    assert t2.min() < t.min() and t2.max() > t.max()                             # ... and outside the observed range


@pytest.mark.parametrize("cid,p", SMALL, ids=[f"{c}-{p}" for c, p in SMALL])
def test_truth_is_the_directional_derivative_of_the_posterior(cid, p):
    """Central differences of the long-double posterior along v at steps h and h / 2 (h = 2^-8), Richardson-combined
    R = (4 D(h/2) - D(h)) / 3.  theta is stored in fp64, so each quotient is compared with the JVP along the direction (a - b) / (2 h)
    its two points really span (the JVP is linear in v).  A missing or mis-signed term errs at order 1 on the mags scale; the
    truncation of R is O(h^4) and the rounding of the long-double posterior, divided by h, sits many orders below 1e-6.  The plain
    central difference's error falls about 4 x from h to h / 2 (checked where it is above the rounding)."""
    c, fam, m, t, y, th, m2, t2 = _inputs(cid, p)
    v = PT.directions(c, p)[0]
    v = v / np.linalg.norm(v)      # (1114 hypers: a unit step keeps h |v| small)

    def quot(step):
        a, b = th + step * v, th - step * v
        u = (a.astype(X) - b.astype(X)) / X(2 * step)
        pa, pb = PT.posterior(*fam, m, t, y, a, m2, t2, X), PT.posterior(*fam, m, t, y, b, m2, t2, X)
        return (pa[0] - pb[0]) / X(2 * step), (pa[1] - pb[1]) / X(2 * step), u

    h = 2.0 ** -8
    (m1, v1, u1), (m2_, v2, u2) = quot(h), quot(h / 2)
    P, alpha = PT.parts(*fam, m, t, y, th, X)
    dm, dv, gm, gv = PT.jvp_from_parts(*fam, m, t, th, m2, t2, P, alpha, (4 * u2 - u1) / 3, X, True)
    sm, sv = PT.scale_of(gm[:, 0]), PT.scale_of(gv[:, 0])
    em = float(np.max(np.abs((4 * m2_ - m1) / 3 - dm[:, 0]) / sm))
    ev = float(np.max(np.abs((4 * v2 - v1) / 3 - dv[:, 0]) / sv))
    # the plain quotients against the JVP along their own directions
    d1 = PT.jvp_from_parts(*fam, m, t, th, m2, t2, P, alpha, u1, X)
    d2 = PT.jvp_from_parts(*fam, m, t, th, m2, t2, P, alpha, u2, X)
    e1 = max(float(np.max(np.abs(m1 - d1[0][:, 0]) / sm)), float(np.max(np.abs(v1 - d1[1][:, 0]) / sv)))
    e2 = max(float(np.max(np.abs(m2_ - d2[0][:, 0]) / sm)), float(np.max(np.abs(v2 - d2[1][:, 0]) / sv)))
    print(f"{cid}:{p} Richardson error mean {em:.2g} var {ev:.2g}; central difference {e1:.2g} -> {e2:.2g} (ratio {e1 / max(e2, 1e-300):.2f})")
    assert em <= 1e-6 and ev <= 1e-6, (em, ev)
    if e1 > 1e-10:
        assert 3.0 <= e1 / e2 <= 5.0, (e1, e2)


@pytest.mark.parametrize("cid,p", [("lmc_sizes", 2), ("lmc_sizes", 4), ("lmc_D24_missing", 0), ("lmc_Q9", 0), ("sm_Q4", 0), ("se", 0)])
def test_scale_direction(cid, p):
    """along information.scale_direction every amplitude grows together: Kdot = 2 K, kdot = 2 k, so dmean . s = 0 and dvar . s = 2 var"""
    c, fam, m, t, y, th, m2, t2 = _inputs(cid, p)
    s = information.scale_direction(*fam, th)
    P, alpha = PT.parts(*fam, m, t, y, th, X)
    dm, dv, gm, gv = PT.jvp_from_parts(*fam, m, t, th, m2, t2, P, alpha, s, X, True)
    var = PT.posterior_from_parts(*fam, m, t, th, m2, t2, P, alpha, X)[1]
    tol = 64 * PT.COND_MAX * EPS
    assert float(np.max(np.abs(dm[:, 0]) / PT.scale_of(gm[:, 0]))) <= tol
    assert float(np.max(np.abs(dv[:, 0] - 2 * var) / PT.scale_of(gv[:, 0]))) <= tol
    assert float(np.max(np.abs(dv[:, 0]))) > 0


@pytest.mark.parametrize("cid,p", [("lmc_sizes", 5), ("lmc_D24_missing", 0), ("sm_Q4", 0), ("se", 0)])
def test_noise_direction_closed_form(cid, p):
    """v = e_{sigma_d}: Kdot = 2 sigma_d^2 diag(m_i == d) and no cross term, so
    dmean_j = -2 sigma_d^2 sum_{m_i = d} w_ij alpha_i,   dvar_j = 2 sigma_d^2 ([m_j == d] + sum_{m_i = d} w_ij^2)"""
    c, fam, m, t, y, th, m2, t2 = _inputs(cid, p)
    kidx, Q, D, R = fam
    n, mm = t.shape[0], t2.shape[0]
    mi = np.asarray(m, np.int64) if kidx == 7 else np.zeros(n, np.int64)
    mj = np.asarray(m2, np.int64) if kidx == 7 else np.zeros(mm, np.int64)
    P, alpha = PT.parts(*fam, m, t, y, th, X)
    W = P @ PT.cross_gram(*fam, m, t, th, m2, t2, X)[0]
    sig2 = T.transform(*fam, th, X)["sig2"]
    for d in sorted({0, int(mi[-1]), (D - 1 if kidx == 7 else 0)}):
        v = np.zeros(th.shape[0])
        v[d] = 1.0
        dm, dv = PT.jvp_from_parts(*fam, m, t, th, m2, t2, P, alpha, v, X)
        sel = (mi == d).astype(X)
        want_m = -2 * sig2[d] * (W.T @ (sel * alpha))
        want_v = 2 * sig2[d] * ((mj == d).astype(X) + (W * W).T @ sel)
        assert float(np.max(np.abs(dm[:, 0] - want_m))) <= 1e3 * EPS * float(np.max(np.abs(want_m)) + 1e-300)
        assert float(np.max(np.abs(dv[:, 0] - want_v))) <= 1e3 * EPS * float(np.max(np.abs(want_v)))


def test_jitter_convention():
    """P and alpha belong to K + k diag(sigma^2); no derivative is scaled by 1 + k"""
    c, fam, m, t, y, th, m2, t2 = _inputs("lmc_sizes", 2)
    V = PT.directions(c, 2)
    P, alpha = PT.parts(*fam, m, t, y, th, X, 1)
    Kj = T.gram(*fam, m, t, th, X, 1)
    assert float(np.abs(P @ Kj - np.eye(t.shape[0])).max()) <= 8 * PT.COND_MAX * t.shape[0] * EPS
    got = PT.jvp(*fam, m, t, y, th, m2, t2, V, X, 1)
    want = PT.jvp_from_parts(*fam, m, t, th, m2, t2, P, alpha, V, X)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.allclose(got[0].astype(np.float64), PT.truth_of(c, 2)[0].astype(np.float64), rtol=1e-6)      # the rounds matter


def test_budget_factor_M_and_caps():
    """Two legitimate fp64 programs within M / 4 of each other on every case the GPU tests use (the jitter case included), every
    budget under its cap, cond(K) <= COND_MAX.  CPU programs only."""
    worst = 0.0
    for cid, p in PT.patients():
        c = PT.case(cid)
        m, t, _ = c["pts"][p]
        assert PT.cond(*PT.fam(c), m, t, c["th"][p]) <= PT.COND_MAX, (cid, p)
        r = PT.programs_of(c, p)
        worst = max(worst, PT.spread(r["eg"]))
        assert PT.budget(r["eg"], PT.M_PJVP) < PT.GRAD_BUDGET_CAP, (cid, p, r["eg"])
        print(f"{cid}:{p} n {t.shape[0]} m {r['truth'][0].shape[0]} E_b {r['eg'][0]:.2g} E_c {r['eg'][1]:.2g} spread {PT.spread(r['eg']):.1f}")
    for p in (2, 4, 5):
        r = PT.programs_of(PT.case("lmc_sizes"), p, 1)
        worst = max(worst, PT.spread(r["eg"]))
        assert PT.budget(r["eg"], PT.M_PJVP) < PT.GRAD_BUDGET_CAP, p

    def rule(s):   # the smallest power of two M with spread <= M / 4
        M = 1
        while s > M / 4:
            M *= 2
        return M

    print(f"spread between the programs: {worst:.1f} -> M_PJVP {max(LG.M_GRAD, rule(worst))}")
    assert worst <= PT.M_PJVP / 4
    assert PT.M_PJVP == max(LG.M_GRAD, rule(worst))


# ---- medgp_amd/sensitivity.py --------------------------------------------------------------------------------------------------------

def _spd(g, k):
    B = g.standard_normal((k, k))
    return B @ B.T + k * np.eye(k)


def test_covariance_factor_against_the_inverse():
    g = T._philox(20261502, 0)
    k = 7
    A = _spd(g, k)
    S = sensitivity.covariance_factor(A)
    assert S.shape == (k, k)
    assert np.abs(S @ S.T - np.linalg.inv(A)).max() <= 1e-12 * np.abs(np.linalg.inv(A)).max()
    # a free subset: the inverse of the restricted matrix on the free rows and columns, zeros elsewhere
    big = np.zeros((k + 2, k + 2))
    free = np.array([True, False] + [True] * (k - 2) + [False, True])
    idx = np.flatnonzero(free)
    big[np.ix_(idx, idx)] = A
    big[1, 1], big[k, k] = -3.0, 0.0
    for fr in (free, idx):
        S = sensitivity.covariance_factor(big, fr)
        C_ = S @ S.T
        assert np.abs(C_[np.ix_(idx, idx)] - np.linalg.inv(A)).max() <= 1e-12 * np.abs(np.linalg.inv(A)).max()
        assert not C_[1].any() and not C_[k].any() and not C_[:, 1].any()
    # a rank cut: the top directions of the covariance = the smallest eigenvalues of the Hessian
    w, U = np.linalg.eigh(A)
    S = sensitivity.covariance_factor(A, rank=3)
    assert S.shape == (k, 3)
    assert np.abs(S @ S.T - (U[:, :3] / w[:3]) @ U[:, :3].T).max() <= 1e-12 / w[0]
    assert np.linalg.eigvalsh(np.linalg.inv(A) - S @ S.T).min() >= -1e-12 / w[0]          # what is cut is positive semi-definite


def test_covariance_factor_refuses_an_indefinite_hessian():
    g = T._philox(20261502, 1)
    A = _spd(g, 5)
    A[2, 2] = -1.0
    with pytest.raises(curvature.NotPositiveDefinite) as e:
        sensitivity.covariance_factor(A)
    assert "not a minimum" in str(e.value)
    with pytest.raises(curvature.NotPositiveDefinite):
        curvature.laplace_evidence(0.0, A)                    # ... where laplace_evidence does
    assert sensitivity.covariance_factor(A, free=[0, 1, 3, 4]).shape == (5, 4)


def test_hyper_variance_is_the_diagonal_of_J_Sigma_Jt():
    g = T._philox(20261502, 2)
    k, m = 6, 9
    A = _spd(g, k)
    J = g.standard_normal((m, k))
    S = sensitivity.covariance_factor(A)
    want = np.diag(J @ np.linalg.inv(A) @ J.T)
    assert np.abs(sensitivity.hyper_variance(J @ S) - want).max() <= 1e-12 * want.max()
    assert sensitivity.hyper_variance(np.zeros((0, 3))).shape == (0,)


@pytest.mark.parametrize("fam,names", [((7, 2, 3, 2), ["noise", "A", "mu", "v", "kappa"]), ((8, 4, 1, 0), ["noise", "w", "mu", "v"]),
                                       ((0, 1, 1, 0), ["noise", "l", "sf"])], ids=["lmc", "sm", "se"])
def test_by_group_slices_the_hypers_of_every_family(fam, names):
    H = T.num_hyp(*fam)
    gs = sensitivity.groups(*fam)
    assert [n for n, _ in gs] == names
    assert gs[0][1].start == 0 and gs[-1][1].stop == H and all(a[1].stop == b[1].start for a, b in zip(gs, gs[1:]))
    kidx, Q, D, R = fam
    if kidx == 7:      # the truth's own layout (nlml_truth.transform)
        assert [s.stop - s.start for _, s in gs] == [D, Q * D * R, Q, Q, Q * D]
    J = np.zeros((2, H))
    for i, (n, s) in enumerate(gs):      # group i gets the constant i + 1 in row 0, one entry 3 in row 1
        J[0, s] = i + 1
        J[1, s.start] = 3.0
    out = sensitivity.by_group(*fam, J)
    for i, (n, s) in enumerate(gs):
        assert abs(out[n][0] - (i + 1)) <= 1e-15 and abs(out[n][1] - 3.0 / np.sqrt(s.stop - s.start)) <= 1e-15
    with pytest.raises(ValueError):
        sensitivity.by_group(*fam, J[:, :-1])


# ---- the ABI surface and the host geometry -------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_posterior_jvp(built_lib):
    src = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    assert re.search(r"int\s+medgp_posterior_jvp_batch\s*\(", src)
    assert "tests/posterior_jvp_truth.py" in src
    assert hasattr(C.CDLL(built_lib), "medgp_posterior_jvp_batch")
    assert "medgp_posterior_jvp_batch" in capi.SYMBOLS
    lib = capi.load()
    assert lib.medgp_abi_version() >= 18
    assert lib.medgp_profile_num_kernels() == 23          # the frozen table
    assert lib.medgp_profile_num_kernels_all() == 29      # ... and the one behind it
    names = [lib.medgp_profile_kernel_name(k).decode() for k in range(lib.medgp_profile_num_kernels_ext())]
    assert names[23:29] == ["k_fc_vec", "k_fc_t", "k_fc_scan", "k_fc_qm", "k_fc_tables", "k_fc_wgrad"]
    assert names[29:34] == ["k_lgo_vec", "k_lgo_inv", "k_lgo_s", "k_lgo_t", "k_lgo_wgrad"]
    assert names[34:38] == ["k_fisher_prep", "k_fisher_kdot", "k_fisher_t", "k_fisher_wgrad"]
    assert names[38:43] == ["k_hess_moments", "k_hess_slabsum", "k_hess_beta", "k_hess_wgrad", "k_hess_epilogue"]
    assert names[43:46] == ["k_pjvp_solve", "k_pjvp_u", "k_pjvp_dir"]          # appended behind id 42
    blob = open(built_lib, "rb").read()
    assert b"k_pjvp_solve" in blob and b"k_pjvp_u" in blob and b"k_pjvp_dir" in blob
    assert hasattr(capi.Context, "posterior_jvp")


def test_null_arguments_are_argument_errors(built_lib):
    """without a context every call is an argument error (-1) before any device work"""
    lib = capi.load()
    slots = np.zeros(1, np.int32)
    th = np.zeros(8)
    off = np.zeros(2, np.int64)
    ip, dp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    a = (slots.ctypes.data_as(ip), th.ctypes.data_as(dp), off.ctypes.data_as(lp))
    d = th.ctypes.data_as(dp)
    assert lib.medgp_posterior_jvp_batch(None, 1, *a, None, None, 1, d, None, None, d, d, None) == -1
    assert lib.medgp_posterior_jvp_batch(None, 1, *a, None, None, 0, d, None, None, d, d, None) == -1
    assert lib.medgp_posterior_jvp_batch(None, 1, None, None, None, None, None, 1, None, None, None, None, None, None) == -1


def test_host_geometry_under_sanitizers():
    """pjvp_tables.h (the tile table, the launch chunks, buffer sizes, class offsets, the capacity rule) against restatements: a
    stand-alone program built with the host compiler under -fsanitize=address,undefined and started as an ordinary child process"""
    subprocess.check_call(["make", "-s", "-C", CSRC, "pjvp_tables_test"])
    out = subprocess.run([os.path.join(CSRC, "pjvp_tables_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pjvp_tables ok" in out.stdout
