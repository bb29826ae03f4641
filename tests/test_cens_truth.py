"""The definition of censored (detection-limit) observations by EP and its fp64 budget, on the CPU: the budget factor M_CENS measured from two fp64 programs that stop
by the DEVICE rule (CENS_TOL) against the long-double truth at the exact fixed point (never from device output), every budget under its cap,
every case converged within half of MEDGP_CENS_MAX_SWEEPS; the truth's gradient against central differences of its own converged nlml;
c = 0 against nlml_truth.nlml_grad; c = 1 against the closed form (EP is exact there); c = 2 against a one-dimensional quadrature of the
bivariate probability (EP's own approximation error, measured and recorded); a BELOW limit moved up never lowers the likelihood; the
tail functions against scipy where it is importable."""
import math

import numpy as np

import cens_truth as CT
import nlml_truth as T

X = np.longdouble


def _runs():
    return [(cid, p, jr) for cid, p in CT.patients() for jr in ((0, 1) if cid == CT.JITTER_CASE and p in CT.JITTER_PS else (0,))]


def test_budget_factor_M_and_caps():
    """M_CENS is the smallest power of two with M / 4 >= the largest spread of the two fp64 programs; every budget is under its cap
    unclipped; both programs and the truth meet the device's stopping rule within half of MEDGP_CENS_MAX_SWEEPS (a condition on the
    inputs), and the two programs take the same number of sweeps"""
    worst, rows, most = 0.0, [], 0
    cs = set()
    for cid, p, jr in _runs():
        c = CT.case(cid)
        r = CT.programs_of(c, p, jr)
        tr = r["truth"]
        assert r["e"] is not None and tr["status"] == jr, (cid, p, jr)
        assert set(r["e"]) == set(CT.OBJ_OUTPUTS + CT.POST_OUTPUTS)
        assert np.any(tr["grad"] != 0) and np.isfinite(float(tr["nlml"]))
        nc = tr["site"].shape[0]
        cs.add(nc)
        assert nc == int(np.sum(c["code"][p] != 0))
        sw = (tr["dev_sweeps"], r["b"]["sweeps"], r["c"]["sweeps"])
        assert None not in sw and max(sw) <= CT.MEDGP_CENS_MAX_SWEEPS // 2, (cid, p, sw)
        assert r["b"]["sweeps"] == r["c"]["sweeps"] and (nc > 0) == (r["b"]["sweeps"] > 0), (cid, p, sw)
        most = max(most, max(sw), tr["sweeps"])
        print(f"CENS-SWEEPS {cid}:{p} jitter {jr} n {c['pts'][p][1].shape[0]} c {nc} ({c['kind'][p]}): truth {tr['sweeps']} (device rule met at {tr['dev_sweeps']}) "
              f"(b) {r['b']['sweeps']} (c) {r['c']['sweeps']}")
        for k, v in r["e"].items():
            sp, bud = CT.spread(v), CT.budget(v, CT.M_CENS)
            print(f"CENS-BUDGET {cid}:{p} jitter {jr} {k}: E_b {v[0]:.3g} E_c {v[1]:.3g} spread {sp:.1f} budget {bud:.3g} cap {CT.cap_of(k):.3g}")
            rows.append((cid, p, jr, k, sp, bud))
            worst = max(worst, sp)
    print(f"CENS-BUDGET largest spread {worst:.1f}, M_CENS {CT.M_CENS}, most sweeps {most}")
    assert {0, 1, 7, 64} <= cs
    assert all(r[4] <= CT.M_CENS / 4 for r in rows), [r for r in rows if r[4] > CT.M_CENS / 4]
    assert worst > CT.M_CENS / 8, "M_CENS is not the smallest power of two"
    assert abs(worst - CT.MEASURED_SPREAD) <= 0.05 * CT.MEASURED_SPREAD, worst
    over = [r for r in rows if not r[5] <= CT.cap_of(r[3])]
    assert not over, over     # (a draw that does not meet the caps is replaced, not the cap: cens_truth.DRAWS)


def test_every_case_batch_carries_the_placements():
    """each case has c = 0, 1, 7 and 64 among its patients; the placements that can go wrong are where they are said to be"""
    for cid in CT.CASE_IDS:
        c = CT.case(cid)
        assert {0, 1, 7, 64} <= {int(np.sum(cd != 0)) for cd in c["code"]}, cid
    c = CT.case("lmc_D3_Q5")
    for p, kind in enumerate(c["kind"]):
        m, t, y = c["pts"][p]
        code, n = c["code"][p], t.shape[0]
        perm = CT.grouping(7, m, n)
        gc = code[perm]                                         # the codes in the grouped order
        if kind in ("edges7", "same7", "full64"):
            assert gc[0] != 0 and gc[n - 1] != 0                # first and last row of the grouped order
            assert np.any(code == CT.BELOW) and np.any(code == CT.ABOVE)
        if kind == "full64":
            assert np.all(gc[[63, 64, 65]] != 0)
        if kind == "cov":
            d = [d for d in range(3) if np.all(code[m == d] != 0) and np.any(m == d)]
            assert len(d) == 1 and set(code[m == d[0]]) == {CT.BELOW, CT.ABOVE}    # every row of one covariate, signs mixed in it
        if kind == "same7":
            rows = np.where(code != 0)[0]
            assert any(t[a] == t[b] and m[a] == m[b] for i, a in enumerate(rows) for b in rows[i + 1:])
    # 8 noise standard deviations on either side: one site at ~0 and a strongly binding one
    c = CT.case("sm_Q3")
    tr = CT.truth_of(c, 1)
    yl = np.asarray(c["pts"][1][2], np.float32).astype(X)[np.where(c["code"][1] != 0)[0]]
    tcav = 1 / tr["imp_var"] - tr["site"][:, 1]
    zc = ((yl - tr["imp_mean"]) / tr["imp_var"] - tr["site"][:, 0]) / np.sqrt(tcav)       # s = +1: all BELOW
    print("CENS-FAR cavity z of the far7 sites", np.asarray(zc, np.float64))
    assert c["kind"][1] == "far7" and zc.max() > 4 and zc.min() < -3
    far = int(np.argmax(zc))
    assert tr["site"][far, 1] < 1e-6 * tr["site_mag"][far, 1] and tr["site"][int(np.argmin(zc)), 1] == tr["site"][:, 1].max()


_SMALL = [("se", 0), ("se", 2), ("sm_Q3", 0), ("sm_Q3", 1), ("lmc_D3_Q5", 0), ("lmc_D3_Q5", 1)]


def test_truth_gradient_against_central_differences():
    """grad of the truth against central differences of the truth's own CONVERGED nlml in long double, on every hyper of the small
    patients (h = 2^-20: truncation ~ h^2, rounding ~ 2^-64 / h).  The sites move with theta; the gradient holds them fixed: the
    implicit terms vanish at the fixed point.  warp_truth's bar: 1e-8 of the scale."""
    h = 2.0 ** -20
    for cid, p in _SMALL:
        c = CT.case(cid)
        m, t, y = c["pts"][p]
        th, code = c["th"][p], c["code"][p]

        def f(th_):
            return CT.objective(*CT.fam(c), m, t, y, th_, code, X, want_grad=False)["nlml"]
        tr = CT.truth_of(c, p)
        fd = np.zeros(th.shape[0], X)
        for i in range(th.shape[0]):
            e = np.zeros_like(th)
            e[i] = h
            fd[i] = (f(th + e) - f(th - e)) / (2 * X(h))
        eg = CT.error_of(fd.astype(np.float64), tr["grad"])
        print(f"CENS-FD {cid}:{p} c {tr['site'].shape[0]} grad {eg:.3g}")
        assert eg <= 1e-8, (cid, p, eg)


def test_no_censored_row_is_the_plain_nlml():
    for cid, p in (("se", 1), ("sm_Q3", 3), ("lmc_D3_Q5", 2), ("lmc_D24", 3)):
        c = CT.case(cid)
        m, t, y = c["pts"][p]
        assert not np.any(c["code"][p])
        _, tn, tg = T.nlml_grad(*CT.fam(c), m, t, y, c["th"][p], X)
        r = CT.truth_of(c, p)
        assert r["sweeps"] == 0 and r["site"].shape == (0, 2)
        # (the quadratic form is |z|^2 here and y^T alpha there: not the same bits)
        assert abs(r["nlml"] - tn) <= 1e-17 * max(abs(tn), 1)
        assert CT.error_of(np.asarray(r["grad"] - tg, np.float64), np.zeros_like(tg), tg) <= 1e-15


def _conditional(c, p, code):
    """(-log N(y_o; 0, K_oo), mean and covariance of the censored rows given the observed ones, limits, s) in long double"""
    m, t, y = c["pts"][p]
    K = T.gram(*CT.fam(c), m, t, c["th"][p], X)
    yy = np.asarray(y, np.float32).astype(X)
    idx, s = CT.codes(code, yy.shape[0])
    o = np.ones(yy.shape[0], bool)
    o[idx] = False
    L = T._chol_columns(K[np.ix_(o, o)])
    Li = T._tri_inverse(L)
    w, V = Li @ yy[o], Li @ K[np.ix_(o, idx)]
    base = (w @ w) / 2 + np.sum(np.log(np.diagonal(L))) + int(o.sum()) * np.log(2 * X(np.float64(T.REF_PI))) / 2
    return base, V.T @ w, K[np.ix_(idx, idx)] - V.T @ V, yy[idx], s.astype(X)


def test_one_censored_row_is_the_closed_form():
    """c = 1: -log N(y_o; 0, K_oo) - log Phi(s (limit - m) / sd).  EP is exact there, and done after one sweep (the second confirms it)"""
    for cid, p in (("se", 0), ("sm_Q3", 0), ("lmc_D3_Q5", 0), ("lmc_D24", 0)):
        c = CT.case(cid)
        code = c["code"][p]
        base, mc, C, lim, s = _conditional(c, p, code)
        want = base - CT.tail(s[0] * (lim[0] - mc[0]) / np.sqrt(C[0, 0]), X)[0]
        r = CT.truth_of(c, p)
        assert r["sweeps"] == 2
        assert abs(r["nlml"] - want) <= 1e-17 * r["nlml_mag"], (cid, p, float(r["nlml"] - want))
        # the imputation is the truncated normal's mean
        zz = s[0] * (lim[0] - mc[0]) / np.sqrt(C[0, 0])
        rr = CT.tail(zz, X)[1]
        assert abs(r["imp_mean"][0] - (mc[0] - s[0] * np.sqrt(C[0, 0]) * rr)) <= 1e-16 * r["imp_mean_mag"][0]


# EP's own approximation error on two censored rows, in units of the nlml: measured here (the test prints every pair) as at most
# EP_GAP_MEASURED, on the pair of sm_Q3:1 that lies 6 h apart (pairs at one time stamp and 10 h apart follow with 7e-7 and 5e-7; pairs
# further apart than the kernel's reach agree to the quadrature's 1e-12).  The assertion is the measurement with a margin of 4.
EP_GAP_MEASURED = 1.12e-6
EP_GAP_MARGIN = 4.0


def _bivariate_nlml(c, p, code):
    base, mc, C, lim, s = _conditional(c, p, code)
    sd1 = np.sqrt(C[0, 0])
    sd21 = np.sqrt(C[1, 1] - C[0, 1] ** 2 / C[0, 0])
    # row 1 = limit_1 - s_1 u, u >= 0: Gauss-Legendre with 64 nodes on each of 64 panels of [0, |limit_1 - m_1| + 12 sd_1]
    umax = float(abs(lim[0] - mc[0]) + 12 * sd1)
    xs, ws = np.polynomial.legendre.leggauss(64)
    xs, ws = xs.astype(X), ws.astype(X)
    tot = X(0)
    for j in range(64):
        a, b = X(umax * j / 64), X(umax * (j + 1) / 64)
        y1 = lim[0] - s[0] * ((a + b) / 2 + (b - a) / 2 * xs)
        dens = np.exp(-((y1 - mc[0]) / sd1) ** 2 / 2) / (sd1 * CT._const(X)[2])
        m2 = mc[1] + C[0, 1] / C[0, 0] * (y1 - mc[0])
        ph = np.array([np.exp(CT.tail(s[1] * (lim[1] - mm) / sd21, X)[0]) for mm in m2])
        tot += (b - a) / 2 * np.sum(ws * dens * ph)
    return base - np.log(tot)


def test_two_censored_rows_against_quadrature():
    worst = 0.0
    for cid, p in (("se", 2), ("sm_Q3", 4), ("lmc_D3_Q5", 1), ("sm_Q3", 1)):
        c = CT.case(cid)
        full = c["code"][p]
        idx = np.where(full != 0)[0]
        for pair in ((0, 1), (2, 3), (1, 2)):
            code = np.zeros_like(full)
            code[idx[list(pair)]] = full[idx[list(pair)]]
            tr = CT.objective(*CT.fam(c), *c["pts"][p], c["th"][p], code, X, want_grad=False)
            gap = float(tr["nlml"] - _bivariate_nlml(c, p, code))
            dt = abs(float(c["pts"][p][1][idx[pair[0]]]) - float(c["pts"][p][1][idx[pair[1]]]))
            print(f"CENS-EP-GAP {cid}:{p} rows {tuple(idx[list(pair)])} {dt:.1f} h apart: EP - exact = {gap:.3g}")
            worst = max(worst, abs(gap))
    print(f"CENS-EP-GAP largest {worst:.3g}")
    assert worst <= EP_GAP_MARGIN * EP_GAP_MEASURED
    assert worst >= EP_GAP_MEASURED / EP_GAP_MARGIN        # (the record stays what is measured)


def test_a_below_limit_moved_up_never_lowers_the_likelihood():
    for cid, p in (("se", 2), ("lmc_D3_Q5", 1), ("sm_Q3", 1)):
        c = CT.case(cid)
        m, t, y = c["pts"][p]
        code = c["code"][p]
        k = np.where(code == CT.BELOW)[0][1]
        vals = []
        for d in (-0.5, 0.0, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0):
            y2 = y.copy()
            y2[k] = np.float32(y[k] + d)
            vals.append(CT.objective(*CT.fam(c), m, t, y2, c["th"][p], code, X, want_grad=False)["nlml"])
        assert all(b <= a + 4 * np.finfo(X).eps * abs(a) for a, b in zip(vals, vals[1:])), (cid, p, [float(v) for v in vals])
        assert vals[-1] < vals[0]


def test_tail_functions():
    """log Phi and phi / Phi down to z = -35: against the asymptotic series far out, against erfc where that is accurate, and against
    scipy.special.log_ndtr where scipy is importable"""
    for z in (-35.0, -30.0, -20.0):
        lz, r = CT.tail(z, X)
        a = 1 / X(z) ** 2
        series = 1 - a + 3 * a ** 2 - 15 * a ** 3 + 105 * a ** 4 - 945 * a ** 5        # Phi(z) ~ phi(z) / |z| * series
        tol = 2 * 10395 * float(a) ** 6                                                 # the first term left out
        assert abs(r * series / -X(z) - 1) <= tol, z
        assert abs(lz - (-X(z) ** 2 / 2 - np.log(-X(z) * CT._const(X)[2]) + np.log(series))) <= tol, z
    for z in np.linspace(-8.0, 8.0, 65):
        lz, r = CT.tail(z, X)
        ref = 0.5 * math.erfc(-z / math.sqrt(2.0))
        assert abs(float(np.exp(lz)) - ref) <= 1e-14 * ref + 1e-300, z       # (erfc itself is 6e-15 off at z = -8)
        assert abs(float(r) - math.exp(-z * z / 2) / math.sqrt(2 * math.pi) / ref) <= 2e-14 * float(r), z
        l64, r64 = CT.tail(z, np.float64)
        assert abs(float(l64 - lz)) <= 1e-14 * max(abs(float(lz)), 1e-300) and abs(float(r64 - r)) <= 1e-14 * float(r)
    try:
        from scipy.special import log_ndtr
    except ImportError:
        return
    for z in np.linspace(-35.0, 8.0, 173):
        ref = float(log_ndtr(z))
        assert abs(float(CT.tail(z, X)[0]) - ref) <= 2e-14 * abs(ref), z     # (scipy's own error above z = 5 is 7e-15)
