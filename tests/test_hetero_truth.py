"""The definition and the budget of the heteroscedastic and robust calls, on the CPU: the budget factor M_HET measured from the two
fp64 programs alone (never from device output) with every budget under its cap; s = 1 against nlml_truth.nlml_grad; the truth's
gradient against central differences of its own nlml; J non-increasing over the sweeps and J >= the exact Student-t nlml; replicated
rows against one row of scale 1 / k; nu = 1e9 against the Gaussian objective; planted outliers; and the host tables under sanitizers."""
import math
import os
import subprocess

import numpy as np

import hetero_truth as HT
import nlml_truth as T
from medgp_amd import robust

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medgp_amd", "csrc")
X = np.longdouble


def _runs():
    return [(cid, p, jr) for cid, p in HT.patients() for jr in ((0, 1) if cid == HT.JITTER_CASE and p in HT.JITTER_PS else (0,))]


def test_budget_factor_M_and_caps():
    """M_HET is the smallest power of two with M / 4 >= the largest spread of the two fp64 programs over every output (the objective,
    the posterior, the robust call at 0, 1 and 5 sweeps), patient and case, zero and one jitter round; every budget is under its cap
    unclipped"""
    worst, rows = 0.0, []
    want = set(HT.OBJ_OUTPUTS + HT.POST_OUTPUTS) | {f"r{k}_{o}" for k in HT.SWEEPS for o in HT.ROB_OUTPUTS}
    for cid, p, jr in _runs():
        c = HT.case(cid)
        r = HT.programs_of(c, p, jr)
        assert r["e"] is not None and r["truth"]["status"] == jr, (cid, p, jr)
        assert set(r["e"]) == want, set(r["e"]) ^ want
        assert np.any(r["truth"]["grad"] != 0) and np.isfinite(float(r["truth"]["nlml"]))
        for k, v in r["e"].items():
            sp, bud = HT.spread(v), HT.budget(v, HT.M_HET)
            print(f"HET-BUDGET {cid}:{p} jitter {jr} n {c['pts'][p][1].shape[0]} {k}: E_b {v[0]:.3g} E_c {v[1]:.3g} spread {sp:.1f} budget {bud:.3g} cap {HT.cap_of(k):.3g}")
            rows.append((cid, p, jr, k, sp, bud))
            worst = max(worst, sp)
    print(f"HET-BUDGET largest spread {worst:.1f}, M_HET {HT.M_HET}")
    assert all(r[4] <= HT.M_HET / 4 for r in rows), [r for r in rows if r[4] > HT.M_HET / 4]
    assert worst > HT.M_HET / 8, "M_HET is not the smallest power of two"
    assert abs(worst - HT.MEASURED_SPREAD) <= 0.05 * HT.MEASURED_SPREAD, worst
    over = [r for r in rows if not r[5] <= HT.cap_of(r[3])]
    assert not over, over     # (a draw that does not meet the caps is replaced, not the cap: hetero_truth.DRAWS)


def test_unit_scales_are_the_plain_nlml():
    """s = 1 on every row: nlml and grad are nlml_truth.nlml_grad's to 1e-17, with zero and one jitter round"""
    for cid, p in HT.patients():
        c = HT.case(cid)
        m, t, y = c["pts"][p]
        n = t.shape[0]
        for jr in (0, 1):
            _, tn, tg = T.nlml_grad(*HT.fam(c), m, t, y, c["th"][p], X, jr)
            r = HT.hetero(*HT.fam(c), m, t, y, c["th"][p], np.ones(n), X, jr)
            assert abs(r["nlml"] - tn) <= 1e-17 * max(abs(tn), 1), (cid, p, jr)
            assert HT.error_of(np.asarray(r["grad"] - tg, np.float64), np.zeros_like(tg), tg) <= 1e-17, (cid, p, jr)


_FD = [("lmc_D3_Q5", 0), ("lmc_D3_Q5", 1), ("se", 0), ("sm_Q3", 0)]


def test_truth_gradient_against_central_differences():
    """the heteroscedastic gradient against central differences of the truth's own nlml in long double, on every hyper of four patients
    (h = 2^-20: truncation ~ h^2, rounding ~ 2^-64 / h)"""
    h = 2.0 ** -20
    for cid, p in _FD:
        c = HT.case(cid)
        m, t, y = c["pts"][p]
        th, s = c["th"][p], c["scale"][p]

        def f(th_):
            return HT.hetero(*HT.fam(c), m, t, y, th_, s, X, want_grad=False)["nlml"]
        tr = HT.hetero(*HT.fam(c), m, t, y, th, s, X)
        fd = np.zeros(th.shape[0], X)
        for i in range(th.shape[0]):
            e = np.zeros_like(th)
            e[i] = h
            fd[i] = (f(th + e) - f(th - e)) / (2 * X(h))
        eg = HT.error_of(fd.astype(np.float64), tr["grad"])
        print(f"HET-FD {cid}:{p} grad {eg:.3g}")
        assert eg <= 1e-8, (cid, p, eg)


def test_bound_is_non_increasing_over_the_sweeps():
    """J(theta, nu, s^(k)) at fixed theta never rises from one E-step to the next (each is the exact minimiser in s of the bound with
    q(f) re-optimised), and the robust call's last value is the trace's last"""
    for cid, p in HT.patients():
        c = HT.case(cid)
        m, t, y = c["pts"][p]
        r = HT.robust(*HT.fam(c), m, t, y, c["th"][p], c["nu"][p], 8, None, X, want_grad=False)
        tr = np.array(r["trace"], X)
        assert np.all(np.diff(tr) <= 1e-15 * np.abs(tr[:-1])), (cid, p, tr)
        assert tr[0] - tr[-1] > 0 and r["obj"] == tr[-1], (cid, p)
        # a warm start from the returned scales with no sweep is the same evaluation
        r0 = HT.robust(*HT.fam(c), m, t, y, c["th"][p], c["nu"][p], 0, r["scale"].astype(np.float64), X, want_grad=False)
        assert abs(r0["obj"] - r["obj"]) <= 1e-15 * abs(r["obj"])


def _student_t_nlml_n2(K, y, sig2, nu):
    """-log of  int int N(y; 0, K + diag(sig2 / tau)) Gamma(tau_1; nu/2, nu/2) Gamma(tau_2; nu/2, nu/2) dtau  for two rows, by the
    trapezoidal rule in u = log tau (the integrand decays doubly exponentially at both ends)"""
    u = np.linspace(-30.0, 12.0, 1681)
    tau = np.exp(u)
    c = nu / 2
    lg = c * math.log(c) - math.lgamma(c) + c * u - c * tau          # log Gamma density times the Jacobian tau
    a11 = K[0, 0] + sig2 / tau[:, None]
    a22 = K[1, 1] + sig2 / tau[None, :]
    det = a11 * a22 - K[0, 1] ** 2
    quad = (a22 * y[0] ** 2 - 2 * K[0, 1] * y[0] * y[1] + a11 * y[1] ** 2) / det
    lp = -0.5 * quad - 0.5 * np.log(det) - math.log(2 * T.REF_PI) + lg[:, None] + lg[None, :]
    mx = lp.max()
    du = u[1] - u[0]
    return -(mx + math.log(np.exp(lp - mx).sum() * du * du))


def test_bound_lies_above_the_exact_student_t_nlml():
    """n = 2 rows on one covariate: J >= the exact Student-t nlml by quadrature, at ones, after 1 and after 20 sweeps, for several nu;
    and the gap closes as the sweeps go on"""
    for nu, y in ((3.0, (0.3, 2.5)), (1.0, (-1.0, 4.0)), (30.0, (0.5, -0.2))):
        t = np.array([0.0, 1.5], np.float32)
        th = np.array([math.log(0.4), math.log(2.0), math.log(1.1)])
        K = T.gram(0, 1, 1, 0, None, t, th, np.float64, -1)
        sig2 = math.exp(th[0]) ** 2
        exact = _student_t_nlml_n2(K, np.array(y), sig2, nu)
        js = [robust.dense(K, np.array(y), sig2, nu, k)["obj"] for k in (0, 1, 20)]
        print(f"HET-BOUND nu {nu}: exact {exact:.6f} J {js}")
        assert all(j >= exact - 1e-9 for j in js), (nu, exact, js)
        assert js[0] >= js[1] >= js[2] and js[2] - exact < js[0] - exact


def test_dense_restatement_agrees_with_the_truth():
    """medgp_amd.robust.dense (float64) on the truth's K: obj, scale, resid, fvar, delta within 1e-9 of the long-double truth"""
    for cid, p in (("lmc_D3_Q5", 1), ("sm_Q3", 0)):
        c = HT.case(cid)
        m, t, y = c["pts"][p]
        n = t.shape[0]
        mm = HT._meta(c["kidx"], m, n)
        K = T.gram(*HT.fam(c), m, t, c["th"][p], np.float64, -1)
        sig2 = np.asarray(T.transform(*HT.fam(c), c["th"][p], np.float64)["sig2"])[mm]
        d = robust.dense(K, y.astype(np.float64), sig2, np.asarray(c["nu"][p])[mm], 3)
        tr = HT.robust(*HT.fam(c), m, t, y, c["th"][p], c["nu"][p], 3, None, X, want_grad=False)
        e = HT.robust_errors(d, tr)
        print(f"HET-DENSE {cid}:{p} {e}")
        assert set(e) == {"obj", "scale", "delta", "resid", "fvar"} and all(v <= 1e-9 for v in e.values()), e


def test_replicates_equal_one_row_of_scale_one_over_k():
    """a row repeated k = 3 times at s = 1 gives the same posterior at test points as one row holding the mean at s = 1 / 3 (the
    replicate values are chosen on a 2^-10 grid so that their mean is a float32 exactly)"""
    c = HT.case("lmc_D3_Q5")
    m, t, y = c["pts"][1]
    th = c["th"][1]
    n = t.shape[0]
    rows = [5, 40]
    keep = np.array([i for i in range(n) if i not in rows])
    mean32 = {i: np.float32(np.round(float(y[i]) * 1024) / 1024) for i in rows}
    reps = {i: np.array([mean32[i], mean32[i] + np.float32(0.125), mean32[i] - np.float32(0.125)], np.float32) for i in rows}
    assert all(float(np.sum(reps[i].astype(np.float64))) == 3 * float(mean32[i]) for i in rows)
    m3 = np.concatenate([m[keep]] + [np.full(3, m[i], m.dtype) for i in rows])
    t3 = np.concatenate([t[keep]] + [np.full(3, t[i], t.dtype) for i in rows])
    y3 = np.concatenate([y[keep]] + [reps[i] for i in rows])
    m1 = np.concatenate([m[keep], m[rows]])
    t1 = np.concatenate([t[keep], t[rows]])
    y1 = np.concatenate([y[keep], np.array([mean32[i] for i in rows], np.float32)])
    s1 = np.concatenate([np.ones(keep.shape[0]), np.full(len(rows), 1.0 / 3.0)])
    m2, t2, _ = HT.points(c, 1)
    a = HT.posterior(*HT.fam(c), m3, t3, y3, th, np.ones(m3.shape[0]), m2, t2, None, X)
    b = HT.posterior(*HT.fam(c), m1, t1, y1, th, s1, m2, t2, None, X)
    # (1 / 3 as a float64 is 2^-54 relative from a third, and three coincident rows make K_s ill-conditioned by 1 / sigma^2: 1e-12)
    em = float(np.max(np.abs(a["mean"] - b["mean"]) / a["mag_mean"]))
    ev = float(np.max(np.abs(a["var"] - b["var"]) / a["mag_var"]))
    print(f"HET-REPLICATES mean {em:.3g} var {ev:.3g}")
    assert em <= 1e-12 and ev <= 1e-12, (em, ev)


def test_huge_nu_reproduces_the_gaussian_objective():
    """nu = 1e9: the scales stay at 1 to (e_i - 1) / nu, kappa(nu, 1) -> 0, and J, its gradient, resid and fvar are the Gaussian call's.
    Tolerance: s - 1 ~ 1e-9 e_i moves nlml by ~ 1e-9 of its gradient in s; lgamma(5e8) ~ 1e10 carries 2^-64 relative in the long double
    (5e-10 absolute per row) -- 1e-6 relative covers both with two orders to spare."""
    for cid, p in (("lmc_D3_Q5", 1), ("se", 0)):
        c = HT.case(cid)
        m, t, y = c["pts"][p]
        n = t.shape[0]
        nd = HT.nout(c["kidx"], c["D"])
        r = HT.robust(*HT.fam(c), m, t, y, c["th"][p], np.full(nd, 1e9), 3, None, X)
        g = HT.hetero(*HT.fam(c), m, t, y, c["th"][p], np.ones(n), X)
        assert np.all(np.abs(r["scale"] - 1) <= 1e-6)
        assert abs(r["obj"] - g["nlml"]) <= 1e-6 * g["nlml_mag"], (cid, p, float(r["obj"] - g["nlml"]))
        assert HT.error_of(r["grad"].astype(np.float64), g["grad"]) <= 1e-6
        assert HT.error_of(r["resid"].astype(np.float64), g["resid"]) <= 1e-6
        assert HT.error_of(r["fvar"].astype(np.float64), g["fvar"], g["fvar_mag"]) <= 1e-6


def _nelder_free_fit(fun, th0, steps=60):
    """plain gradient descent with backtracking on a scalar objective fun(theta) -> (value, grad)"""
    th = th0.copy()
    v, g = fun(th)
    lr = 0.05
    for _ in range(steps):
        while True:
            cand = th - lr * g
            v2, g2 = fun(cand)
            if np.isfinite(v2) and v2 <= v:
                th, v, g, lr = cand, v2, g2, lr * 1.5
                break
            lr *= 0.5
            if lr < 1e-8:
                return th
    return th


def test_planted_outliers_are_set_aside():
    """5 rows of an n = 120 SE patient moved by 8 noise sd: every planted row's final scale exceeds every clean row's, and the
    posterior of the theta learned under Student-t noise is nearer the clean-data posterior than the Gaussian fit's.  On the truth's
    float64 program, verified here before any device sees it."""
    g = T._philox(20262104, 0)
    n, nu = 120, 4.0
    t = np.sort(g.uniform(0.0, 100.0, size=n)).astype(np.float32)
    th_true = np.array([math.log(0.3), math.log(8.0), math.log(1.0)])
    fam = (0, 1, 1, 0)
    K = T.gram(*fam, None, t, th_true, np.float64, -1)
    f = np.linalg.cholesky(K + 1e-10 * np.eye(n)) @ g.standard_normal(n)
    y_clean = (f + 0.3 * g.standard_normal(n)).astype(np.float32)
    planted = g.choice(n, size=5, replace=False)
    y = y_clean.copy()
    y[planted] += (8 * 0.3 * np.where(g.uniform(size=5) < 0.5, -1.0, 1.0)).astype(np.float32)
    clean = np.setdiff1d(np.arange(n), planted)

    def gauss(th, yy=y):
        r = HT.hetero(*fam, None, t, yy, th, np.ones(n), np.float64)
        return float(r["nlml"]), r["grad"]

    state = {"s": None}

    def rob(th):
        r = HT.robust(*fam, None, t, y, th, [nu], 2, state["s"], np.float64)
        state["s"] = np.asarray(r["scale"], np.float64)
        return float(r["obj"]), r["grad"]
    th0 = np.array([math.log(0.5), math.log(5.0), math.log(0.8)])
    th_g = _nelder_free_fit(gauss, th0)
    th_r = _nelder_free_fit(rob, th0)
    th_c = _nelder_free_fit(lambda th: gauss(th, y_clean), th0)
    fin = HT.robust(*fam, None, t, y, th_r, [nu], 20, None, np.float64)
    s = np.asarray(fin["scale"], np.float64)
    print(f"HET-OUTLIERS planted scales {np.sort(s[planted])} largest clean {s[clean].max():.3f}; sigma gauss {math.exp(th_g[0]):.3f} robust {math.exp(th_r[0]):.3f} clean {math.exp(th_c[0]):.3f}")
    assert s[planted].min() > s[clean].max(), (s[planted], s[clean].max())
    t2 = np.linspace(0.0, 100.0, 101).astype(np.float32)
    zero = np.zeros(t2.shape[0])
    ref = HT.posterior(*fam, None, t, y_clean, th_c, np.ones(n), None, t2, zero, np.float64)["mean"]
    pg = HT.posterior(*fam, None, t, y, th_g, np.ones(n), None, t2, zero, np.float64)["mean"]
    pr = HT.posterior(*fam, None, t, y, th_r, s, None, t2, zero, np.float64)["mean"]
    dg, dr = float(np.sqrt(np.mean((pg - ref) ** 2))), float(np.sqrt(np.mean((pr - ref) ** 2)))
    print(f"HET-OUTLIERS rms distance to the clean-data posterior mean: gaussian {dg:.4f} robust {dr:.4f}")
    assert dr < dg, (dr, dg)
    w = robust.outlier_weight(s)
    assert w[planted].max() < w[clean].min()


def test_hetero_and_robust_tables_walk_clean_under_sanitizers():
    for name in ("hetero_tables_test", "robust_tables_test"):
        subprocess.check_call(["make", "-s", "-C", CSRC, name])
        out = subprocess.run([os.path.join(CSRC, name)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert f"{name}: ok" in out.stdout
