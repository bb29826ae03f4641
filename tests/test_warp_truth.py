"""The definition and the budget of the warp calls, on the CPU: the budget factor M_WARP measured from the two fp64 programs alone
(never from device output) with every budget under its cap; the truth's grad and dpsi against central differences of its nlml in
long double; psi = 0 and kind NONE against nlml_truth.nlml_grad; the quantiles through g; lpd as the derivative of the predictive CDF;
the host tables under sanitizers; and how far medgp_amd.warp.moments at 32 nodes lies from a dense quadrature (recorded, not a bar)."""
import math
import os
import subprocess

import numpy as np

import nlml_truth as T
import warp_truth as WT
from medgp_amd import warp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medgp_amd", "csrc")
X = np.longdouble


def _runs():
    return [(cid, p, jr) for cid, p in WT.patients() for jr in ((0, 1) if cid == WT.JITTER_CASE and p in WT.JITTER_PS else (0,))]


def test_budget_factor_M_and_caps():
    """M_WARP is the smallest power of two with M / 4 >= the largest spread of the two fp64 programs; every budget is under its cap
    unclipped; the truth has non-zero grad and dpsi"""
    worst, rows = 0.0, []
    for cid, p, jr in _runs():
        c = WT.case(cid)
        r = WT.programs_of(c, p, jr)
        assert r["e"] is not None and r["truth"]["status"] == jr, (cid, p, jr)
        assert set(r["e"]) == set(WT.OBJ_OUTPUTS + WT.POST_OUTPUTS)
        assert np.any(r["truth"]["grad"] != 0) and np.isfinite(float(r["truth"]["nlml"]))
        if c["kind"] is None or np.any(c["kind"] == WT.SAS):
            assert np.any(r["truth"]["dpsi"] != 0)
        for k, v in r["e"].items():
            sp, bud = WT.spread(v), WT.budget(v, WT.M_WARP)
            print(f"WARP-BUDGET {cid}:{p} jitter {jr} n {c['pts'][p][1].shape[0]} {k}: E_b {v[0]:.3g} E_c {v[1]:.3g} spread {sp:.1f} budget {bud:.3g} cap {WT.cap_of(k):.3g}")
            rows.append((cid, p, jr, k, sp, bud))
            worst = max(worst, sp)
    print(f"WARP-BUDGET largest spread {worst:.1f}, M_WARP {WT.M_WARP}")
    assert all(r[4] <= WT.M_WARP / 4 for r in rows), [r for r in rows if r[4] > WT.M_WARP / 4]
    assert worst > WT.M_WARP / 8, "M_WARP is not the smallest power of two"
    assert abs(worst - WT.MEASURED_SPREAD) <= 0.05 * WT.MEASURED_SPREAD, worst
    over = [r for r in rows if not r[5] <= WT.cap_of(r[3])]
    assert not over, over     # (a draw that does not meet the caps is replaced, not the cap: warp_truth.DRAWS)


_SMALL = [("se", 0), ("se", 1), ("sm_Q3", 0), ("sm_Q3", 1), ("lmc_D3_Q5", 0), ("lmc_D3_Q5", 1), ("lmc_D3_Q5", 3), ("lmc_D3_mixed", 0)]


def test_truth_gradients_against_central_differences():
    """grad and dpsi of the truth against central differences of the truth's nlml in long double, on every hyper of the small cases
    (h = 2^-20: truncation ~ h^2, rounding ~ 2^-64 / h)"""
    h = 2.0 ** -20
    for cid, p in _SMALL:
        c = WT.case(cid)
        m, t, y = c["pts"][p]
        th, psi = c["th"][p], c["psi"][p]

        def f(th_, psi_):
            return WT.objective(*WT.fam(c), m, t, y, th_, psi_, c["kind"], X, want_grad=False)["nlml"]
        tr = WT.objective(*WT.fam(c), m, t, y, th, psi, c["kind"], X)
        fd = np.zeros(th.shape[0], X)
        for i in range(th.shape[0]):
            e = np.zeros_like(th)
            e[i] = h
            fd[i] = (f(th + e, psi) - f(th - e, psi)) / (2 * X(h))
        eg = WT.error_of(fd.astype(np.float64), tr["grad"])
        fp = np.zeros(psi.shape, X)
        for d in range(psi.shape[0]):
            for k in range(3):
                e = np.zeros_like(psi)
                e[d, k] = h
                fp[d, k] = (f(th, psi + e) - f(th, psi - e)) / (2 * X(h))
        sas = np.ones(psi.shape[0], bool) if c["kind"] is None else c["kind"] == WT.SAS
        assert not np.any(tr["dpsi"][~sas]) and not np.any(fp[~sas])
        ep = WT.error_of(fp.astype(np.float64), tr["dpsi"], tr["dpsi_mag"])
        print(f"WARP-FD {cid}:{p} grad {eg:.3g} dpsi {ep:.3g}")
        assert eg <= 1e-8 and ep <= 1e-8, (cid, p, eg, ep)


def test_identity_warps_are_the_plain_nlml():
    """kind all NONE: z carries y's long-double bits and the objective is nlml_truth.nlml_grad's; psi = 0: the same to the rounding of
    sinh(asinh(y)).  (The quadratic form is |w|^2 here and y^T alpha there: not the same bits.)"""
    for cid, p in (WT.ZERO_PSI, ("se", 1), ("sm_Q3", 1), ("lmc_D3_mixed", 0)):
        c = WT.case(cid)
        m, t, y = c["pts"][p]
        nd = WT.nout(c["kidx"], c["D"])
        _, tn, tg = T.nlml_grad(*WT.fam(c), m, t, y, c["th"][p], X)
        none = WT.objective(*WT.fam(c), m, t, y, c["th"][p], c["psi"][p], np.zeros(nd, np.int64), X, want_parts=True)
        zero = WT.objective(*WT.fam(c), m, t, y, c["th"][p], np.zeros((nd, 3)), None, X, want_parts=True)
        assert np.array_equal(none["parts"]["z"], np.asarray(y, np.float32).astype(X))
        assert none["logjac"] == 0 and not np.any(none["dpsi"]) and not np.any(none["parts"]["lj"])
        assert np.all(np.abs(zero["parts"]["z"] - np.asarray(y, np.float32).astype(X)) <= 4 * np.finfo(X).eps * np.abs(y))
        for r, tol in ((none, 1e-17), (zero, 1e-16)):
            assert abs(r["nlml"] - tn) <= tol * max(abs(tn), 1)
            assert WT.error_of(np.asarray(r["grad"] - tg, np.float64), np.zeros_like(tg), tg) <= 100 * tol
        assert abs(zero["logjac"]) <= 1e-16 * float(zero["logjac_mag"])


def test_quantiles_go_back_through_g_and_lpd_is_the_density():
    """g(quant_k) = zmean + zq_k sd in the truth; lpd = log d/dy Phi((g(y) - zmean) / sd) by a central difference in y"""
    for cid, p in (("sm_Q3", 1), ("lmc_D3_Q5", 2), ("lmc_D3_mixed", 0), ("lmc_D24", 1)):
        c = WT.case(cid)
        post = WT.truth_of(c, p)["post"]
        m2, t2, y2 = WT.points(c, p)
        mm = WT._meta(c["kidx"], m2, t2.shape[0])
        sd = np.sqrt(post["zvar"])
        for k, zq in enumerate(c["zq"]):
            back = WT.warp(post["quant"][:, k], mm, c["psi"][p], c["kind"], X)[0]
            want = post["zmean"] + X(zq) * sd
            assert np.all(np.abs(back - want) <= 1e-15 * np.maximum(np.abs(want), sd)), (cid, p, k)
        assert np.all(np.diff(post["quant"], axis=1) > 0)

        def cdf(yv):
            g = WT.warp(yv, mm, c["psi"][p], c["kind"], X)[0]
            return np.array([0.5 * math.erfc(-float(v) / math.sqrt(2.0)) for v in (g - post["zmean"]) / sd])
        yy = np.asarray(y2, np.float32).astype(np.float64)
        h = 1e-5 * np.maximum(np.abs(yy), 1.0)
        dens = (cdf(yy + h) - cdf(yy - h)) / (2 * h)
        ok = dens > 1e-6                      # (far in a tail the difference of two CDF values carries no digits)
        assert ok.sum() >= 12
        assert np.all(np.abs(np.log(dens[ok]) - post["lpd"][ok].astype(np.float64)) <= 1e-5), (cid, p)


def test_warp_tables_walk_clean_under_sanitizers():
    subprocess.check_call(["make", "-s", "-C", CSRC, "warp_tables_test"])
    out = subprocess.run([os.path.join(CSRC, "warp_tables_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "warp_tables_test: ok" in out.stdout


def _dense_moments(zmean, zvar, psi, kind, m2):
    """mean and variance of g^-1(N(zmean, zvar)) by the trapezoidal rule on 20001 points over +- 12 sd (exponentially convergent for
    an analytic integrand that has decayed to nothing at the ends)"""
    x = np.linspace(-12.0, 12.0, 20001)
    w = np.exp(-x * x / 2)
    w /= w.sum()
    zz = zmean[:, None] + np.sqrt(zvar)[:, None] * x[None, :]
    yy = warp.inverse(zz, psi, kind, None if m2 is None else np.repeat(np.asarray(m2)[:, None], x.shape[0], axis=1))
    mean = yy @ w
    return mean, ((yy - mean[:, None]) ** 2) @ w


def test_moments_rule_against_dense_quadrature():
    """medgp_amd.warp.moments at 32 nodes against a dense quadrature over the case set: printed and recorded
    (warp_truth.MOMENTS_MEASURED), not a bar -- the assertion only holds the record to what is measured"""
    worst = dict(all=[0.0, 0.0], delta_ge_075=[0.0, 0.0])
    for cid, p in WT.patients():
        c = WT.case(cid)
        post = WT.truth_of(c, p)["post"]
        m2, _, _ = WT.points(c, p)
        zm, zv = post["zmean"].astype(np.float64), post["zvar"].astype(np.float64)
        mean, var = warp.moments(zm, zv, c["psi"][p], c["kind"], m2)
        dm, dv = _dense_moments(zm, zv, c["psi"][p], c["kind"], m2)
        em, es = np.abs(mean - dm) / np.sqrt(dv), np.abs(np.sqrt(var) - np.sqrt(dv)) / np.sqrt(dv)
        mm = WT._meta(c["kidx"], m2, zm.shape[0])
        sas = np.ones(mm.shape[0], bool) if c["kind"] is None else (c["kind"] == WT.SAS)[mm]
        wide = (np.exp(c["psi"][p][mm, 2]) >= 0.75) | ~sas
        print(f"WARP-MOMENTS {cid}:{p} mean {em.max():.3g} sd {es.max():.3g} (delta >= 0.75: mean {em[wide].max() if wide.any() else 0:.3g} sd {es[wide].max() if wide.any() else 0:.3g})")
        worst["all"] = [max(worst["all"][0], em.max()), max(worst["all"][1], es.max())]
        if wide.any():
            worst["delta_ge_075"] = [max(worst["delta_ge_075"][0], em[wide].max()), max(worst["delta_ge_075"][1], es[wide].max())]
    print("WARP-MOMENTS worst", worst)
    for key in worst:
        for got, rec in zip(worst[key], WT.MOMENTS_MEASURED[key]):
            assert got <= 2 * rec and got >= rec / 2, (key, worst, WT.MOMENTS_MEASURED)
