"""medgp_hess_vec without a GPU: the long-double truth (hess_truth.py) against Richardson differences of the gradient the suite
already trusts (nlml_truth.nlml_grad), its symmetry, the scale identity, the five-moment block form against the naive per-hyper
form, the conditions under which the truth's fp64 error budget may be used to judge the device (test_hess_gpu.py),
medgp_amd/curvature.py on the truth's matvec, the ABI surface, and the host geometry's own test program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from medgp_amd import capi, curvature, information, synth
import fisher_truth as F
import hess_truth as HT
import loo_grad_truth as LG
import nlml_truth as T
from random_patients import random_patient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medgp_amd", "csrc")
X = np.longdouble
EPS = float(np.finfo(X).eps)
SMALL_N = 23


def _small(kidx):
    g = T._philox(20261402, kidx)
    n = SMALL_N
    if kidx == 7:
        Q, D, R = 2, 3, 2
        m, t, y = random_patient(g, D, n, "plain")
    else:
        Q, D, R = (3, 1, 0) if kidx == 8 else (1, 1, 0)
        m, t = None, np.sort(g.uniform(0.0, 200.0, size=n)).astype(np.float32)
        y = g.standard_normal(n).astype(np.float32)
    th = synth.theta(4719, kidx, kidx, Q, D, R)
    return (kidx, Q, D, R), m, t, y, th, g.standard_normal((2, th.shape[0]))


KERNELS = pytest.mark.parametrize("kidx", [7, 8, 0], ids=["lmc", "sm", "se"])


@KERNELS
def test_truth_is_the_directional_derivative_of_the_gradient(kidx):
    """Central differences of nlml_truth.nlml_grad along v at steps h, 2 h, 4 h (h = 2^-11), Richardson-extrapolated:
    R(h) = (4 D(h) - D(2h)) / 3 has truncation error O(h^4), R(2h) 16 times that, so |R(2h) - R(h)| bounds the error of R(h) from the
    steps alone -- no chosen constant.  theta is stored in fp64, so the quotient is compared with H along the direction
    (a - b) / (2 h) the two points really span (H v is linear in v).  Rounding: the long-double gradient carries a few thousand eps
    (cond(K) n, and the cosine's argument), divided by h: 2^16 eps max|g| / h, orders below the truncation term.  Zero jitter rounds.
    The bound must itself be small against H v: the check has teeth.  Worst |R(h) - Hv| / max|Hv| observed: 6e-11 (LMC-SM), bound 9.1e-10."""
    fam, m, t, y, th, V = _small(kidx)
    v = V[0]

    def quot(step):
        a, b = th + step * v, th - step * v
        u = (a.astype(X) - b.astype(X)) / X(2 * step)
        return (T.nlml_grad(*fam, m, t, y, a, X)[2] - T.nlml_grad(*fam, m, t, y, b, X)[2]) / X(2 * step), u

    h = 2.0 ** -11
    (d1, u1), (d2, u2), (d4, u4) = quot(h), quot(2 * h), quot(4 * h)
    r1, r2 = (4 * d1 - d2) / 3, (4 * d2 - d4) / 3
    hv, g = HT.hess_vec(*fam, m, t, y, th, (4 * u1 - u2) / 3, X, want_grad=True)
    hv = hv[0]
    g0 = T.nlml_grad(*fam, m, t, y, th, X)[2]
    assert float(np.abs(g - g0).max()) <= 64 * EPS * float(np.abs(g0).max())      # the gradient output is nlml_grad's
    scale = float(np.abs(hv).max())
    tol = float(np.abs(r2 - r1).max()) + 2.0 ** 16 * EPS * float(np.abs(g0).max()) / h
    err = float(np.abs(r1 - hv).max())
    print(f"kernel {kidx}: |R(h) - Hv| / max|Hv| = {err / scale:.2g}, bound {tol / scale:.2g}")
    assert tol <= 1e-6 * scale, (tol, scale)
    assert err <= tol, (err, tol)


@KERNELS
def test_symmetry(kidx):
    """u . H v = v . H u to long-double rounding: both products use the same P and alpha, the identity holds for any symmetric P"""
    fam, m, t, y, th, V = _small(kidx)
    hv = HT.hess_vec(*fam, m, t, y, th, V, X)
    a, b = np.sum(V[0].astype(X) * hv[1]), np.sum(V[1].astype(X) * hv[0])
    mag = float(np.linalg.norm(V[0]) * np.linalg.norm(hv[1].astype(np.float64)) + np.linalg.norm(V[1]) * np.linalg.norm(hv[0].astype(np.float64)))
    assert float(abs(a - b)) <= 1e-15 * mag, (float(a), float(b))


@pytest.mark.parametrize("cid,p", [("lmc_sizes", 1), ("lmc_sizes", 4), ("lmc_Q9", 0), ("sm_Q4", 0), ("se", 0)])
def test_scale_identity(cid, p):
    c = HT.case(cid)
    m, t, y = c["pts"][p]
    n = t.shape[0]
    fam, th = HT.fam(c), c["th"][p]
    s = information.scale_direction(*fam, th)
    P, alpha, _ = HT.parts(*fam, m, t, y, th, X)
    hs, g = HT.hess_from_parts(*fam, m, t, th, P, alpha, s, X)
    want = 2 * np.sum(np.asarray(y, np.float32).astype(X) * alpha)
    got = HT.scale_identity(fam, th, s, hs[0], g)
    mag = float(np.sum(np.abs(s.astype(X) * hs[0]))) + abs(float(want))
    assert abs(float(got - want)) <= 8 * HT.COND_MAX * n * EPS * mag, (float(got), float(want))


def test_block_form_equals_the_naive_per_hyper_form():
    """the five-moment form (S, SM, SV, M3, M4) against one n x n second-derivative matrix per hyper, LMC-SM with empty covariates too"""
    fam, m, t, y, th, V = _small(7)
    a = HT.hess_vec(*fam, m, t, y, th, V, X, form="naive")
    b = HT.hess_vec(*fam, m, t, y, th, V, X, form="blocks")
    assert float(np.abs(a - b).max()) <= 1e-16 * float(np.abs(a).max())
    c = HT.case("lmc_sizes")
    m, t, y = c["pts"][2]
    V = HT.directions(c, 2)
    a = HT.hess_vec(*HT.fam(c), m, t, y, c["th"][2], V, X, form="naive")
    b = HT.hess_vec(*HT.fam(c), m, t, y, c["th"][2], V, X, form="blocks")
    assert float(np.abs(a - b).max()) <= 1e-16 * float(np.abs(a).max())


@pytest.mark.parametrize("rounds", [1, 3])
def test_jitter_convention(rounds):
    """P and alpha belong to K + k diag(sigma^2); every kernel derivative is that of the un-jittered K"""
    c = HT.case("lmc_sizes")
    p = 2
    m, t, y = c["pts"][p]
    fam, th = HT.fam(c), c["th"][p]
    n = t.shape[0]
    P, alpha, _ = HT.parts(*fam, m, t, y, th, X, rounds)
    Kj = T.gram(*fam, m, t, th, X, rounds)
    assert float(np.abs(P @ Kj - np.eye(n)).max()) <= 8 * HT.COND_MAX * n * EPS
    assert float(np.abs(Kj @ alpha - np.asarray(y, np.float32).astype(X)).max()) <= 8 * HT.COND_MAX * n * EPS * float(np.abs(y).max())
    V = HT.directions(c, p)
    got = HT.hess_vec(*fam, m, t, y, th, V, X, rounds)
    want = HT.hess_from_parts(*fam, m, t, th, P, alpha, V, X)[0]
    assert np.array_equal(got, want)
    assert not np.allclose(got.astype(np.float64), HT.truth_of(c, p)[0].astype(np.float64), rtol=1e-6)      # the rounds matter


def test_budget_factor_M_and_caps():
    """The conditions of test_fisher.py for the Hessian products: two legitimate fp64 programs within M / 4 of each other on every case
    the GPU tests use (jitter cases included), every budget under its cap, cond(K) <= COND_MAX.  CPU programs only."""
    worst = 0.0
    for cid in HT.CASE_IDS:
        c = HT.case(cid)
        for p, (m, t, _) in enumerate(c["pts"]):
            assert HT.cond(*HT.fam(c), m, t, c["th"][p]) <= HT.COND_MAX, (cid, p)
            r = HT.programs_of(c, p)
            worst = max(worst, HT.spread(r["eg"]))
            assert HT.budget(r["eg"], HT.M_HESS) < HT.GRAD_BUDGET_CAP, (cid, p, r["eg"])
            print(f"{cid}:{p} n {t.shape[0]} E_b {r['eg'][0]:.2g} E_c {r['eg'][1]:.2g} spread {HT.spread(r['eg']):.1f}")
    for rounds in (1, 3):
        for p in (2, 4, 5):
            r = HT.programs_of(HT.case("lmc_sizes"), p, rounds)
            worst = max(worst, HT.spread(r["eg"]))
            assert HT.budget(r["eg"], HT.M_HESS) < HT.GRAD_BUDGET_CAP, (p, rounds)

    def rule(s):   # the smallest power of two M with spread <= M / 4
        M = 1
        while s > M / 4:
            M *= 2
        return M

    print(f"spread between the programs: {worst:.1f} -> M_HESS {max(LG.M_GRAD, rule(worst))}")
    assert worst <= HT.M_HESS / 4
    assert HT.M_HESS == max(LG.M_GRAD, rule(worst))


# ---- medgp_amd/curvature.py ---------------------------------------------------------------------------------------------------------

def _prior_grad(flag, typ, p0, p1, is_exp, theta):
    """what prior_apply (kernels_core.h) adds to the gradient, restated in long double: -d log p / d theta, 0 without a prior, and a
    clamp's pinned hyper contributes nothing here (its whole gradient is zeroed)"""
    th = np.asarray(theta).astype(X)
    g = np.zeros_like(th)
    for h in range(th.shape[0]):
        if not flag[h] or typ[h] not in (1, 2):
            continue
        hv = np.exp(th[h]) if is_exp[h] else th[h]
        if typ[h] == 1:
            dlp = -(hv - X(p0[h])) / X(p1[h])
        else:
            dlp = X(0) if hv == p0[h] else -np.sign(hv - X(p0[h])) / X(p1[h])
        g[h] = -(hv * dlp if is_exp[h] else dlp)
    return g


def test_prior_curvature_against_differences_of_the_prior_gradient():
    g = T._philox(20261403, 0)
    H = 12
    flag = np.array([1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 0], np.uint8)
    typ = np.array([1, 1, 2, 2, 1, 0, 1, 2, -1, 1, 2, 2], np.int32)
    is_exp = np.array([1, 0, 1, 0, 1, 1, 1, 1, 1, 0, 0, 1], np.uint8)
    p0 = g.uniform(0.2, 1.5, H).astype(np.float32)
    p1 = g.uniform(0.3, 2.0, H).astype(np.float32)
    th = g.uniform(-1.0, 1.0, H)
    diag, free = curvature.prior_curvature(flag, typ, p0, p1, is_exp, th)
    assert np.array_equal(free, np.arange(H) != 5) and diag[5] == 0.0          # the clamp pins hyper 5
    assert not diag[[4, 8, 11]].any()                                           # no prior (flag 0 / unknown type)
    assert diag[3] == 0.0 and diag[10] == 0.0                                   # Laplace, not exp: no curvature away from the kink
    assert diag[2] != 0.0                                                       # Laplace under exp: the chain rule's term
    h = 2.0 ** -12
    for k in range(H):
        e = np.zeros(H)
        e[k] = h
        d1 = (_prior_grad(flag, typ, p0, p1, is_exp, th + e)[k] - _prior_grad(flag, typ, p0, p1, is_exp, th - e)[k]) / X(2 * h)
        d2 = (_prior_grad(flag, typ, p0, p1, is_exp, th + 2 * e)[k] - _prior_grad(flag, typ, p0, p1, is_exp, th - 2 * e)[k]) / X(4 * h)
        r1 = (4 * d1 - d2) / 3
        tol = float(abs(d2 - d1)) + 1e-12      # (|R(h) - f''| <= |D(2h) - D(h)|: the truncation of D(h) alone is a third of it)
        assert abs(float(r1) - diag[k]) <= tol, (k, float(r1), diag[k], tol)
    # at the kink of a Laplace prior: slope 0 by the gradient's convention, and no curvature
    d0, _ = curvature.prior_curvature([1], [2], [1.0], [0.5], [1], [0.0])
    assert d0[0] == 0.0


def test_newton_step_on_a_planted_indefinite_quadratic():
    g = T._philox(20261404, 0)
    H = 9
    U, _ = np.linalg.qr(g.standard_normal((H, H)))
    lam_pd = np.linspace(0.5, 4.0, H)
    lam_in = lam_pd.copy()
    lam_in[3] = -1.0
    Hpd, Hin = (U * lam_pd) @ U.T, (U * lam_in) @ U.T
    Fm = (U * np.abs(lam_in)) @ U.T
    rhs = g.standard_normal((2, H))
    mats = [Hpd, Hin]

    def hess_mv(V):
        return np.stack([V[b] @ mats[b].T for b in range(2)])

    def fisher_mv(V):
        return np.stack([V[b] @ Fm.T for b in range(V.shape[0])])

    x, used, its, conv = curvature.newton_step(hess_mv, fisher_mv, rhs, tol=1e-12, max_iter=4 * H)
    assert list(used) == [False, True] and conv.all() and (its > 0).all()
    assert np.abs(x[0] - np.linalg.solve(Hpd, rhs[0])).max() <= 1e-9 * np.abs(x[0]).max()          # the Newton step where H is PD
    assert np.abs(x[1] - np.linalg.solve(Fm, rhs[1])).max() <= 1e-9 * np.abs(x[1]).max()           # the Fisher step where it is not
    assert float(rhs[1] @ x[1]) > 0                                                                 # -x is a descent direction


def test_newton_step_on_the_truth_matvec():
    """the n = 63 LMC case: whichever matrix the step took, it solves that matrix's system, and -x descends"""
    c = HT.case("lmc_sizes")
    m, t, y = c["pts"][2]
    fam, th = HT.fam(c), c["th"][2]
    H = th.shape[0]
    hmv = HT.matvec_of(*fam, m, t, y, th, np.float64)
    fmv = F.matvec_of(*fam, m, t, th, np.float64)
    g = HT.truth_of(c, 2)[1].astype(np.float64)[None, :]
    Hm = information.fisher_matrix(hmv, H)[0]
    Fm = information.fisher_matrix(fmv, H)[0]
    lam = 1e-3 * np.trace(Fm) / H
    x, used, its, conv = curvature.newton_step(hmv, fmv, g, damping=lam, tol=1e-10, max_iter=8 * H)
    pd = np.linalg.eigvalsh(Hm + lam * np.eye(H)).min() > 0
    assert conv[0] and (not used[0] or not pd)          # a PD Hessian never triggers the fall-back
    want = np.linalg.solve((Fm if used[0] else Hm) + lam * np.eye(H), g[0])
    assert np.abs(x[0] - want).max() <= 1e-6 * np.abs(want).max()
    assert float(g[0] @ x[0]) > 0
    assert hasattr(curvature, "bind")


def test_laplace_evidence_on_a_gaussian_toy():
    """exp(-nlml) = exp(-c - 1/2 (x - m)^T A (x - m)): the integral is exp(-c) (2 pi)^(k/2) det(A)^(-1/2), which Laplace gives exactly"""
    g = T._philox(20261405, 0)
    k = 4
    B = g.standard_normal((k, k))
    A = B @ B.T + k * np.eye(k)
    c0 = 1.7
    want = -c0 + 0.5 * k * np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(A)[1]
    assert abs(curvature.laplace_evidence(c0, A) - want) <= 1e-12 * abs(want)
    # a pinned hyper drops out of rows and columns
    big = np.zeros((k + 1, k + 1))
    big[:k, :k] = A
    big[k, k] = -3.0
    free = np.array([True] * k + [False])
    assert abs(curvature.laplace_evidence(c0, big, free) - want) <= 1e-12 * abs(want)
    assert abs(curvature.laplace_evidence(c0, big, np.arange(k)) - want) <= 1e-12 * abs(want)
    with pytest.raises(curvature.NotPositiveDefinite) as e:      # not a minimum: it says so
        curvature.laplace_evidence(c0, big)
    assert "not a minimum" in str(e.value)


# ---- the ABI surface and the host geometry -------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_hess_vec(built_lib):
    src = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    assert re.search(r"int\s+medgp_hess_vec\s*\(", src)
    assert "tests/hess_truth.py" in src
    assert "Out of scope: the exact (observed) Hessian" not in src
    assert hasattr(C.CDLL(built_lib), "medgp_hess_vec")
    assert "medgp_hess_vec" in capi.SYMBOLS
    lib = capi.load()
    assert lib.medgp_abi_version() >= 17
    assert lib.medgp_profile_num_kernels() == 23          # the frozen table
    assert lib.medgp_profile_num_kernels_all() == 29      # ... and the one behind it
    names = [lib.medgp_profile_kernel_name(k).decode() for k in range(lib.medgp_profile_num_kernels_ext())]
    assert names[23:29] == ["k_fc_vec", "k_fc_t", "k_fc_scan", "k_fc_qm", "k_fc_tables", "k_fc_wgrad"]
    assert names[29:34] == ["k_lgo_vec", "k_lgo_inv", "k_lgo_s", "k_lgo_t", "k_lgo_wgrad"]
    assert names[34:38] == ["k_fisher_prep", "k_fisher_kdot", "k_fisher_t", "k_fisher_wgrad"]
    assert {"k_hess_moments", "k_hess_slabsum", "k_hess_beta", "k_hess_wgrad", "k_hess_epilogue"} <= set(names[38:])      # appended behind them
    blob = open(built_lib, "rb").read()
    assert b"k_hess_moments" in blob and b"k_hess_beta" in blob and b"k_hess_wgrad" in blob and b"k_hess_epilogue" in blob
    assert hasattr(capi.Context, "hess_vec")


def test_null_arguments_are_argument_errors(built_lib):
    lib = capi.load()
    slots = np.zeros(1, np.int32)
    th = np.zeros(8)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    assert lib.medgp_hess_vec(None, 1, slots.ctypes.data_as(ip), th.ctypes.data_as(dp), 1, th.ctypes.data_as(dp), th.ctypes.data_as(dp), None, None) == -1


def test_host_geometry_under_sanitizers():
    """hess_tables.h (buffer sizes, class offsets, grids, the capacity rule) against restatements: a stand-alone program built with the
    host compiler under -fsanitize=address,undefined and started as an ordinary child process"""
    subprocess.check_call(["make", "-s", "-C", CSRC, "hess_tables_test"])
    out = subprocess.run([os.path.join(CSRC, "hess_tables_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "hess_tables ok" in out.stdout
