"""medgp_fisher_vec without a GPU: the long-double truth (fisher_truth.py) against difference quotients of the Gram matrix, against
the W -> g map the suite already trusts (the adjoint identity), its symmetry, sign, scale direction and jitter convention, the
conditions under which the truth's fp64 error budget may be used to judge the device (test_fisher_gpu.py), medgp_amd/information.py
on the truth's matvec, the ABI surface, and the host geometry's own test program."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from medgp_amd import capi, information, synth
import fisher_truth as F
import loo_grad_truth as LG
import nlml_truth as T
from random_patients import random_patient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medgp_amd", "csrc")
X = np.longdouble
EPS = float(np.finfo(X).eps)
SMALL_N = 24


def _small(kidx):
    g = T._philox(20261302, kidx)
    n = SMALL_N
    if kidx == 7:
        Q, D, R = 2, 3, 2
        m, t, _ = random_patient(g, D, n, "plain")
    else:
        Q, D, R = (3, 1, 0) if kidx == 8 else (1, 1, 0)
        m, t = None, np.sort(g.uniform(0.0, 200.0, size=n)).astype(np.float32)
    th = synth.theta(4719, kidx, kidx, Q, D, R)
    return (kidx, Q, D, R), m, t, th, g.standard_normal((2, th.shape[0]))


KERNELS = pytest.mark.parametrize("kidx", [7, 8, 0], ids=["lmc", "sm", "se"])


@KERNELS
def test_kdot_is_the_directional_derivative_of_the_gram_matrix(kidx):
    """Central differences of nlml_truth.gram along v at steps h and 2 h, Richardson-extrapolated: R(h) = (4 D(h) - D(2h)) / 3 has
    truncation error O(h^4), so R(2h) carries 16 times that of R(h) and |R(2h) - R(h)| bounds the error of R(h) from the steps alone.
    theta is stored in fp64, so the two evaluation points are rounded; the quotient is compared with Kdot along the direction
    (a - b) / (2 h) they really span (exact in long double).  Rounding: an entry of K carries eps |w dt| from the argument of its
    cosine (|w dt| up to 2 pi mu 200 h, a few thousand radians: 2^12 allows for it), divided by h.  The bound must itself be small
    against Kdot: the check has teeth."""
    fam, m, t, th, V = _small(kidx)
    v = V[0]

    def quot(step):
        a, b = th + step * v, th - step * v
        u = (a.astype(X) - b.astype(X)) / X(2 * step)
        return (T.gram(*fam, m, t, a, X) - T.gram(*fam, m, t, b, X)) / X(2 * step), u

    h = 2.0 ** -20     # (h |w dt| ~ 1e-3 .. 1e-2: the truncation term of R(h) is its fourth power)
    (d1, u1), (d2, u2), (d4, u4) = quot(h), quot(2 * h), quot(4 * h)
    r1, r2 = (4 * d1 - d2) / 3, (4 * d2 - d4) / 3
    Kd = F.dgram_dir(*fam, m, t, th, (4 * u1 - u2) / 3, X)     # (Kdot is linear in the direction)
    scale = float(np.abs(Kd).max())
    kmax = float(np.abs(T.gram(*fam, m, t, th, X)).max())
    tol = float(np.abs(r2 - r1).max()) + 2.0 ** 12 * EPS * kmax / h
    err = float(np.abs(r1 - Kd).max())
    print(f"kernel {kidx}: |R(h) - Kdot| / max|Kdot| = {err / scale:.2g}, bound {tol / scale:.2g}")
    assert tol <= 1e-8 * scale, (tol, scale)
    assert err <= tol, (err, tol)
    assert float(np.abs(Kd - Kd.T).max()) == 0.0 or float(np.abs(Kd - Kd.T).max()) <= 4 * EPS * scale


@KERNELS
def test_adjoint_identity_ties_kdot_to_the_w_to_g_map(kidx):
    """v . grad_from_w(W) = 1/2 sum W o Kdot for a random symmetric W: Kdot is the adjoint of the W -> g map the gradient tests hold to
    the reference.  Both sides are sums of at most 4 n^2 Q products in long double: the bound is that many roundings of the sums of
    the magnitudes."""
    fam, m, t, th, V = _small(kidx)
    g = T._philox(20261303, kidx)
    W = g.standard_normal((SMALL_N, SMALL_N)).astype(X)
    W = (W + W.T) / 2
    gw = LG.grad_from_w(*fam, m, t, th, W, X, "naive")
    for v in V:
        Kd = F.dgram_dir(*fam, m, t, th, v, X)
        lhs, rhs = np.sum(v.astype(X) * gw), np.sum(W * Kd) / 2
        mag = float(np.sum(np.abs(v.astype(X) * gw)) + np.sum(np.abs(W * Kd)) / 2)
        assert float(abs(lhs - rhs)) <= 4 * SMALL_N ** 2 * fam[1] * EPS * mag, (float(lhs), float(rhs))
    if kidx == 7:      # ... and the block-sum form of the map, which the larger patients take
        gb = LG.grad_from_w(*fam, m, t, th, W, X, "blocks")
        assert float(np.abs(gb - gw).max()) <= 1e-16 * float(np.abs(gw).max())


@KERNELS
def test_symmetry_and_sign(kidx):
    """u . F v = v . F u and v . F v > 0.  Both products use the same P, and the identity holds for ANY symmetric P: the difference is
    the rounding of the products alone (n-term sums in long double, a few hundred eps); 1e-15 of the magnitudes leaves a factor 100."""
    fam, m, t, th, V = _small(kidx)
    Fv = F.fisher_vec(*fam, m, t, th, V, X)
    a, b = np.sum(V[0].astype(X) * Fv[1]), np.sum(V[1].astype(X) * Fv[0])
    mag = float(np.linalg.norm(V[0]) * np.linalg.norm(Fv[1].astype(np.float64)) + np.linalg.norm(V[1]) * np.linalg.norm(Fv[0].astype(np.float64)))
    assert float(abs(a - b)) <= 1e-15 * mag, (float(a), float(b))
    for j in range(2):
        assert float(np.sum(V[j].astype(X) * Fv[j])) > 0


@pytest.mark.parametrize("cid,p", [("lmc_sizes", 1), ("lmc_sizes", 4), ("lmc_Q9", 0), ("sm_Q4", 0), ("se", 0)])
def test_scale_direction(cid, p):
    """Along s every amplitude grows together: Kdot = 2 K (the un-jittered K), so F s = grad_from_w(2 P) and s^T F s = 2 n.  The first
    is exact up to the rounding of Kdot; the second goes through P K = I, which the long-double inverse meets to cond n eps."""
    c = F.case(cid)
    m, t, _ = c["pts"][p]
    n = t.shape[0]
    fam = F.fam(c)
    s = information.scale_direction(*fam, c["th"][p])
    K0 = T.gram(*fam, m, t, c["th"][p], X)
    Kd = F.dgram_dir(*fam, m, t, c["th"][p], s, X)
    assert float(np.abs(Kd - 2 * K0).max()) <= 64 * EPS * float(np.abs(K0).max())
    P = F.inverse(*fam, m, t, c["th"][p], X)
    Fs = F.fisher_from_inverse(*fam, m, t, c["th"][p], P, s, X)[0]
    ref = LG.grad_from_w(*fam, m, t, c["th"][p], 2 * P, X, "naive")
    assert float(np.abs(Fs - ref).max()) <= 8 * F.COND_MAX * n * EPS * float(np.abs(ref).max())
    sFs = float(np.sum(s.astype(X) * Fs))
    assert abs(sFs - 2 * n) <= 8 * F.COND_MAX * n * EPS * 2 * n, (sFs, 2 * n)


def test_no_dependence_on_y():
    """The truth takes no y at all; the cases' y (another seed's draw would change it) never reaches it."""
    for fn in (F.dgram_dir, F.inverse, F.fisher_vec, F.fisher_vec_linalg, F.matvec_of):
        assert "y" not in inspect.signature(fn).parameters
    c = F.case("lmc_sizes")
    m, t, y = c["pts"][2]
    a = F.truth_of(c, 2)
    c2 = dict(c, pts=[(mm, tt, -2 * yy) for mm, tt, yy in c["pts"]])
    b = F.fisher_vec(*F.fam(c2), *c2["pts"][2][:2], c2["th"][2], F.directions(c, 2), X)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("rounds", [1, 3])
def test_jitter_convention(rounds):
    """P is the inverse of the jittered matrix K + k diag(sigma^2); Kdot is the derivative of the UN-jittered K: along log sigma_d it is
    2 sigma_d^2 on covariate d's diagonal entries, not (1 + k) times that."""
    c = F.case("lmc_sizes")
    p = 2
    m, t, _ = c["pts"][p]
    fam, th = F.fam(c), c["th"][p]
    n = t.shape[0]
    P = F.inverse(*fam, m, t, th, X, rounds)
    Kj = T.gram(*fam, m, t, th, X, rounds)
    assert float(np.abs(P @ Kj - np.eye(n)).max()) <= 8 * F.COND_MAX * n * EPS
    K0 = T.gram(*fam, m, t, th, X, 0)
    h = T.transform(*fam, th, X)
    assert float(np.abs((Kj - K0) - rounds * np.diag(h["sig2"][np.asarray(m)])).max()) <= 4 * EPS * float(np.abs(Kj).max())
    V = F.directions(c, p)
    got = F.fisher_vec(*fam, m, t, th, V, X, rounds)
    want = F.fisher_from_inverse(*fam, m, t, th, P, V, X)
    assert np.array_equal(got, want)
    assert not np.allclose(got.astype(np.float64), F.truth_of(c, p).astype(np.float64), rtol=1e-6)      # the rounds matter
    for d in range(fam[2]):
        e = np.zeros(th.shape[0])
        e[d] = 1.0
        Kd = F.dgram_dir(*fam, m, t, th, e, X)
        assert np.array_equal(Kd, np.diag(np.where(np.asarray(m) == d, 2 * h["sig2"][d], X(0))))


def test_budget_factor_M_and_caps():
    """The conditions of test_loo_grad.py for the Fisher products: two legitimate fp64 programs within M / 4 of each other on every case
    the GPU tests use (jitter cases included), every budget under its cap, cond(K) <= COND_MAX.  CPU programs only."""
    worst = 0.0
    for cid in F.CASE_IDS:
        c = F.case(cid)
        for p, (m, t, _) in enumerate(c["pts"]):
            assert F.cond(*F.fam(c), m, t, c["th"][p]) <= F.COND_MAX, (cid, p)
            r = F.programs_of(c, p)
            worst = max(worst, F.spread(r["eg"]))
            assert F.budget(r["eg"], F.M_FISHER) < F.GRAD_BUDGET_CAP, (cid, p, r["eg"])
            print(f"{cid}:{p} n {t.shape[0]} E_b {r['eg'][0]:.2g} E_c {r['eg'][1]:.2g} spread {F.spread(r['eg']):.1f}")
    for rounds in (1, 3):
        for p in (2, 4, 5):
            r = F.programs_of(F.case("lmc_sizes"), p, rounds)
            worst = max(worst, F.spread(r["eg"]))
            assert F.budget(r["eg"], F.M_FISHER) < F.GRAD_BUDGET_CAP, (p, rounds)

    def rule(s):   # the smallest power of two M with spread <= M / 4
        M = 1
        while s > M / 4:
            M *= 2
        return M

    print(f"spread between the programs: {worst:.1f} -> M_FISHER {max(LG.M_GRAD, rule(worst))}")
    assert worst <= F.M_FISHER / 4
    assert F.M_FISHER == max(LG.M_GRAD, rule(worst))


# ---- medgp_amd/information.py on the truth's matvec ---------------------------------------------------------------------------------

def _lmc63():
    c = F.case("lmc_sizes")
    m, t, _ = c["pts"][2]
    return c, m, t, c["th"][2], T.num_hyp(*F.fam(c))


def test_fisher_matrix_is_the_matrix_of_unit_products():
    c, m, t, th, H = _lmc63()
    mv = F.matvec_of(*F.fam(c), m, t, th, np.float64)
    calls = []

    def counted(V):
        calls.append(np.asarray(V).shape)
        return mv(V)

    Fm = information.fisher_matrix(counted, H)[0]
    assert calls == [(1, H, H)]                        # one call
    cols = np.array([mv(np.eye(H)[None, h:h + 1])[0, 0] for h in range(H)])
    assert np.array_equal(Fm, (cols + cols.T) / 2)
    assert np.abs(cols - cols.T).max() <= 1e-10 * np.abs(cols).max()
    free = np.array([0, 3, 7, 24])
    Ff = information.fisher_matrix(mv, H, free)[0]
    assert Ff.shape == (4, 4) and np.allclose(Ff, Fm[np.ix_(free, free)], rtol=0, atol=1e-12 * np.abs(Fm).max())
    assert np.linalg.eigvalsh(Fm).min() >= -1e-10 * np.abs(Fm).max()


def test_solve_reproduces_a_dense_solve():
    c, m, t, th, H = _lmc63()
    one = F.matvec_of(*F.fam(c), m, t, th, np.float64)
    Fm = information.fisher_matrix(one, H)[0]
    lam = 1e-3 * np.trace(Fm) / H
    g = T._philox(20261304, 0).standard_normal((3, H))
    g[2] = 0.0                                         # a patient that is done before it starts

    def mv(V):                                         # three "patients" with the same F, batched
        return np.concatenate([one(V[b:b + 1]) for b in range(V.shape[0])])

    x, its, conv = information.solve(mv, g, damping=lam, tol=1e-12, max_iter=4 * H)
    want = np.linalg.solve(Fm + lam * np.eye(H), g.T).T
    assert conv.all() and its[2] == 0 and np.array_equal(x[2], np.zeros(H)) and (its[:2] > 0).all()
    assert np.abs(x - want).max() <= 1e-8 * np.abs(want).max()
    x1, its1, _ = information.solve(mv, g[:1], damping=lam, tol=1e-12, max_iter=4 * H)
    assert np.array_equal(x1[0], x[0]) and its1[0] == its[0]          # a patient's iterates do not depend on its batch-mates


def test_stderr_handles_a_rank_deficient_matrix():
    """the D = 24 case: covariates without observations give exact zero rows and columns of F"""
    c = F.case("lmc_D24_missing")
    m, t, _ = c["pts"][0]
    kidx, Q, D, R = F.fam(c)
    H = T.num_hyp(kidx, Q, D, R)
    empty = np.flatnonzero(np.bincount(m, minlength=D) == 0)
    seen = np.flatnonzero(np.bincount(m, minlength=D) > 0)
    assert empty.size >= 1
    d0, d1 = int(empty[0]), int(seen[0])
    o_k = D + Q * (D * R + 2)
    free = np.array([d0, d1, D + d0 * R, D + d1 * R, D + Q * D * R, D + Q * D * R + Q, o_k + d0, o_k + d1])
    mv = F.matvec_of(kidx, Q, D, R, m, t, c["th"][0], np.float64)
    Fm = information.fisher_matrix(mv, H, free)[0]
    dead = [0, 2, 6]
    assert not Fm[dead].any() and not Fm[:, dead].any()          # exact zeros
    se, rank = information.stderr(Fm)
    assert rank == 5 and np.isfinite(se).all()
    live = [1, 3, 4, 5, 7]
    want = np.sqrt(np.diag(np.linalg.inv(Fm[np.ix_(live, live)])))
    assert np.allclose(se[live], want, rtol=1e-8)
    assert not se[dead].any()                          # the pseudo-inverse's zeros, exactly
    se1, rank1 = information.stderr(np.ones((2, 2)))   # rank-deficient without a zero row: pinv = ones / 4
    assert rank1 == 1 and np.allclose(se1, [0.5, 0.5])
    se2, rank2 = information.stderr(np.diag([4.0, 1.0]))
    assert rank2 == 2 and np.allclose(se2, [0.5, 1.0])


def test_scale_direction_layout():
    th = synth.theta(1, 2, 7, 2, 3, 2)
    s = information.scale_direction(7, 2, 3, 2, th)
    assert np.array_equal(s[:3], np.ones(3)) and np.array_equal(s[3:15], th[3:15]) and not s[15:19].any() and np.array_equal(s[19:], 2 * np.ones(6))
    assert np.array_equal(information.scale_direction(8, 2, 1, 0, np.zeros(7)), [1, 2, 2, 0, 0, 0, 0])
    assert np.array_equal(information.scale_direction(0, 1, 1, 0, np.zeros(3)), [1, 0, 1])


# ---- the ABI surface and the host geometry -------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_fisher_vec(built_lib):
    src = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    assert re.search(r"int\s+medgp_fisher_vec\s*\(", src)
    assert "tests/fisher_truth.py" in src
    assert hasattr(C.CDLL(built_lib), "medgp_fisher_vec")
    assert "medgp_fisher_vec" in capi.SYMBOLS
    lib = capi.load()
    assert lib.medgp_abi_version() >= 16
    assert lib.medgp_profile_num_kernels() == 23          # the frozen table
    assert lib.medgp_profile_num_kernels_all() == 29      # ... and the one behind it
    names = [lib.medgp_profile_kernel_name(k).decode() for k in range(lib.medgp_profile_num_kernels_ext())]
    assert {"k_fisher_prep", "k_fisher_kdot", "k_fisher_t", "k_fisher_wgrad"} <= set(names[29:])      # appended behind both
    assert names[23:29] == ["k_fc_vec", "k_fc_t", "k_fc_scan", "k_fc_qm", "k_fc_tables", "k_fc_wgrad"]
    assert names[29:34] == ["k_lgo_vec", "k_lgo_inv", "k_lgo_s", "k_lgo_t", "k_lgo_wgrad"]
    blob = open(built_lib, "rb").read()
    assert b"k_fisher_kdot" in blob and b"k_fisher_t" in blob and b"k_fisher_wgrad" in blob
    assert hasattr(capi.Context, "fisher_vec") and hasattr(information, "bind")


def test_null_arguments_are_argument_errors(built_lib):
    lib = capi.load()
    slots = np.zeros(1, np.int32)
    th = np.zeros(8)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    assert lib.medgp_fisher_vec(None, 1, slots.ctypes.data_as(ip), th.ctypes.data_as(dp), 1, th.ctypes.data_as(dp), th.ctypes.data_as(dp), None) == -1


def test_host_geometry_under_sanitizers():
    """fisher_tables.h (tile maps, buffer sizes, the capacity rule) against restatements: a stand-alone program built with the host
    compiler under -fsanitize=address,undefined and started as an ordinary child process"""
    subprocess.check_call(["make", "-s", "-C", CSRC, "fisher_tables_test"])
    out = subprocess.run([os.path.join(CSRC, "fisher_tables_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fisher_tables ok" in out.stdout
