"""CPU checks of tests/mean_truth.py, the definition medgp_mean_nlml_grad / medgp_mean_posterior_batch are held to: its two forms
agree, its gradients are the derivatives of its own nlml, its limits and invariances hold, the budget factor is what the CPU programs
measure, and the host-side geometry of the calls (mean_tables.h) walks clean under sanitizers.  No GPU."""
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mean_truth as MT   # noqa: E402
import nlml_truth as T    # noqa: E402

X = np.longdouble
EPS = float(np.finfo(X).eps)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "medgp_amd", "csrc")


def _small(kidx=7, n=40, seed=5):
    """(fam, meta, t, y, theta, b0, lam > 0) of one small patient, D = 3; y on a 2^-10 grid (sums with grid offsets stay exact in float32)"""
    from medgp_amd import synth
    from random_patients import random_patient
    Q, D, R = (2, 3, 2) if kidx == 7 else (2, 1, 0)
    g = T._philox(20261711, 10 * kidx + seed)
    if kidx == 7:
        m, t, y = random_patient(g, D, n, "plain")
    else:
        m, t, y = None, np.sort(g.uniform(0, 200, n)).astype(np.float32), g.standard_normal(n).astype(np.float32)
    y = (np.round(y.astype(np.float64) * 1024) / 1024 + 0.75).astype(np.float32)
    nd = MT.nout(kidx, D)
    return (kidx, Q, D, R), m, t, y, synth.theta(4717, seed, kidx, Q, D, R), 0.5 * g.standard_normal(nd), g.uniform(0.05, 3.0, nd)


def _rel(a, b):
    a, b = np.asarray(a, X), np.asarray(b, X)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), X(1e-300)))


def test_woodbury_equals_dense_gram():
    """all lam_d > 0: nlml, W~, alpha~ and the posterior of the Woodbury form are those of the zero-mean GP on K~ = K + H Lambda^-1 H^T"""
    for kidx in (7, 8, 0):
        fam, m, t, y, th, b0, lam = _small(kidx)
        for jr in (0, 2):
            w = MT.woodbury(*fam, m, t, y, th, MT.MARGINAL, b0, lam, X, jr, want_parts=True)
            d = MT.dense(*fam, m, t, y, th, b0, lam, X, jr)
            assert abs(w["nlml"] - d["nlml"]) <= 1e-15 * abs(d["nlml"])
            assert _rel(w["parts"]["W"], d["W"]) <= 1e-13 and _rel(w["parts"]["alpha_t"], d["alpha_t"]) <= 1e-13
            g = T._philox(20261712, kidx)
            m2 = g.integers(0, fam[2], 9).astype(np.int32) if kidx == 7 else None
            t2 = g.uniform(-20, 220, 9).astype(np.float32)
            p = MT.posterior(*fam, m, t, y, th, MT.MARGINAL, b0, lam, m2, t2, X, jr)
            dm, dv = MT.dense_posterior(*fam, m, t, y, th, b0, lam, m2, t2, X, jr)
            assert _rel(p["mean"], dm) <= 1e-13 and _rel(p["var"], dv) <= 1e-13
            assert np.all(p["extra"] >= 0) and np.all(p["var"] >= p["var0"])


def test_quadratic_form_is_the_definitions_difference():
    """|w - G delta|^2 + sum lam delta^2 == r0^T P r0 - c^T A^-1 c to the rounding of the two terms, also where they nearly cancel
    (small lam, b0 far from the data)"""
    fam, m, t, y, th, b0, lam = _small(7)
    for b, lm in ((b0, lam), (b0 + 1e3, lam * 1e-6), (b0 - 50.0, np.array([0.0, 1e-9, 2.0]))):
        w = MT.woodbury(*fam, m, t, y, th, MT.MARGINAL, b, lm, X, want_parts=True)["parts"]
        a, c = w["quad_def"]
        assert abs(w["quad"] - (a - c)) <= 64 * EPS * (abs(a) + abs(c))
        assert w["quad"] >= 0


def _richardson(f, x, i, h):
    """(R(h), bound): central differences at h, 2h, 4h; R(h) = (4 D(h) - D(2h)) / 3 has truncation error O(h^4), R(2h) 16 times that,
    so |R(2h) - R(h)| bounds the error of R(h) from the two extrapolation levels alone; rounding adds 8 eps |f| / h"""
    def cd(s):
        a, b = x.copy(), x.copy()
        a[i] += s
        b[i] -= s
        return (f(a) - f(b)) / (X(a[i]) - X(b[i]))
    d1, d2, d4 = cd(h), cd(2 * h), cd(4 * h)
    r1, r2 = (4 * d1 - d2) / 3, (4 * d2 - d4) / 3
    return r1, abs(r2 - r1) + 8 * EPS * abs(f(x)) / h


def test_theta_gradient_is_the_derivative_of_the_truths_own_nlml():
    for kidx, mode in ((7, MT.MARGINAL), (7, MT.FIXED), (8, MT.MARGINAL), (0, MT.MARGINAL)):
        fam, m, t, y, th, b0, lam = _small(kidx, n=24)
        lam = lam.copy()
        lam[0] = 0.0   # one flat covariate
        r = MT.woodbury(*fam, m, t, y, th, mode, b0, lam, X)
        f = lambda x: MT.woodbury(*fam, m, t, y, x, mode, b0, lam, X, want_grad=False)["nlml"]   # noqa: E731
        scale = float(np.abs(r["grad"]).max())
        for i in range(th.shape[0]):
            d, bound = _richardson(f, th, i, 2.0 ** -20)   # (h |w dt| ~ 1e-3 .. 1e-2 on the frequency lines: see tests/test_fisher.py)
            assert bound <= 1e-9 * scale, (kidx, mode, i, float(bound), scale)   # the check has teeth
            assert abs(d - r["grad"][i]) <= bound + 1e-15 * scale, (kidx, mode, i, float(d), float(r["grad"][i]), float(bound))


def test_dmean_and_prior_grad_are_derivatives():
    from medgp_amd import baseline
    fam, m, t, y, th, b0, lam = _small(7, n=24)
    for mode in (MT.MARGINAL, MT.FIXED):
        r = MT.woodbury(*fam, m, t, y, th, mode, b0, lam, X, want_grad=False)
        fb = lambda x: MT.woodbury(*fam, m, t, y, th, mode, x, lam, X, want_grad=False)["nlml"]   # noqa: E731
        for d in range(3):
            v, bound = _richardson(fb, b0, d, 2.0 ** -10)
            assert abs(v - r["dmean"][d]) <= bound + 1e-14 * float(np.abs(r["dmean"]).max())
    r = MT.woodbury(*fam, m, t, y, th, MT.MARGINAL, b0, lam, X, want_grad=False)
    db, dl = MT.prior_grad(r["beta"], r["beta_cov"], b0, lam)
    assert np.all(db == r["dmean"])
    fl = lambda x: MT.woodbury(*fam, m, t, y, th, MT.MARGINAL, b0, np.exp(x), X, want_grad=False)["nlml"]   # noqa: E731
    for d in range(3):
        v, bound = _richardson(fl, np.log(lam), d, 2.0 ** -10)
        assert abs(v - dl[d]) <= bound + 1e-12 * float(np.abs(dl).max()), (d, float(v), float(dl[d]), float(bound))
    # the library's helper restates it in float64; a flat covariate has zero lines
    lam0 = lam.copy()
    lam0[1] = 0.0
    r0 = MT.woodbury(*fam, m, t, y, th, MT.MARGINAL, b0, lam0, X, want_grad=False)
    hb, hl = baseline.prior_grad(r0["beta"].astype(np.float64), r0["beta_cov"].astype(np.float64), b0, lam0)
    tb, tl = MT.prior_grad(r0["beta"], r0["beta_cov"], b0, lam0)
    assert hb[1] == 0 and hl[1] == 0 and r0["dmean"][1] == 0
    assert _rel(hb, tb) <= 1e-14 and _rel(hl, tl) <= 1e-13


def test_fixed_zero_mean_is_the_plain_nlml():
    for kidx in (7, 8, 0):
        fam, m, t, y, th, b0, lam = _small(kidx)
        for jr in (0, 1):
            r = MT.woodbury(*fam, m, t, y, th, MT.FIXED, np.zeros_like(b0), None, X, jr)
            st, nl, g = T.nlml_grad(*fam, m, t, y, th, X, jr)
            assert r["status"] == st == jr
            assert abs(r["nlml"] - nl) <= 1e-17 * abs(nl) and _rel(r["grad"], g) <= 1e-15
            assert np.all(r["beta"] == 0) and np.all(r["beta_cov"] == 0)


def test_large_precision_approaches_the_fixed_mean():
    fam, m, t, y, th, b0, lam = _small(7)
    big = np.full(3, 1e12)
    a = MT.woodbury(*fam, m, t, y, th, MT.MARGINAL, b0, big, X)
    f = MT.woodbury(*fam, m, t, y, th, MT.FIXED, b0, None, X)
    assert abs(a["nlml"] - f["nlml"]) <= 1e-9 * abs(f["nlml"])     # O(n / lam)
    assert _rel(a["grad"], f["grad"]) <= 1e-9 and _rel(a["dmean"], f["dmean"]) <= 1e-9 and _rel(a["beta"], b0) <= 1e-9
    assert np.abs(a["beta_cov"] - np.diag(1 / big.astype(X))).max() <= 1e-20


def test_flat_prior_is_invariant_under_constant_shifts():
    """lam = 0: y -> y + H c leaves nlml and gradient alone and moves beta^ by c (c and y on a 2^-10 grid: the shifted data are exact
    in float32)"""
    fam, m, t, y, th, b0, _ = _small(7)
    c = np.array([3.5, -1.25, 0.0625])
    y2 = (y.astype(np.float64) + c[np.asarray(m)]).astype(np.float32)
    assert np.all(y2.astype(np.float64) == y.astype(np.float64) + c[np.asarray(m)])
    a = MT.woodbury(*fam, m, t, y, th, MT.MARGINAL, b0, np.zeros(3), X)
    b = MT.woodbury(*fam, m, t, y2, th, MT.MARGINAL, b0, np.zeros(3), X)
    assert abs(a["nlml"] - b["nlml"]) <= 1e-14 * abs(a["nlml"]) and _rel(b["grad"], a["grad"]) <= 1e-13
    assert np.abs((b["beta"] - a["beta"]) - c).max() <= 1e-14
    assert np.all(a["dmean"] == 0) and np.all(b["dmean"] == 0)


def test_covariate_without_observations():
    fam, m, t, y, th, b0, lam = _small(7)
    keep = np.asarray(m) != 1
    m1, t1, y1 = np.asarray(m)[keep], t[keep], y[keep]
    r = MT.woodbury(*fam, m1, t1, y1, th, MT.MARGINAL, b0, lam, X)
    assert r["status"] == 0 and r["beta"][1] == X(b0[1]) and r["dmean"][1] == 0
    e = np.zeros(3, X)
    e[1] = 1 / X(lam[1])
    assert np.abs(r["beta_cov"][1] - e).max() <= 1e-18 and np.abs(r["beta_cov"][:, 1] - e).max() <= 1e-18
    # the predictive variance at a point of that covariate gains 1 / lam_d beside the other covariates' share
    p = MT.posterior(*fam, m1, t1, y1, th, MT.MARGINAL, b0, lam, np.array([1], np.int32), np.array([50.0], np.float32), X)
    pf = MT.posterior(*fam, m1, t1, y1, th, MT.FIXED, b0, None, np.array([1], np.int32), np.array([50.0], np.float32), X)
    assert p["extra"][0] >= 1 / X(lam[1]) and p["var0"][0] == pf["var"][0]
    lam0 = lam.copy()
    lam0[1] = 0.0
    assert MT.woodbury(*fam, m1, t1, y1, th, MT.MARGINAL, b0, lam0, X)["status"] == -1
    assert MT.posterior(*fam, m1, t1, y1, th, MT.MARGINAL, b0, lam0, np.array([1], np.int32), np.array([50.0], np.float32), X)["status"] == -1
    assert MT.woodbury(*fam, m1, t1, y1, th, MT.FIXED, b0, None, X)["status"] == 0           # FIXED ignores lam
    assert MT.woodbury(*fam, m[:2], t[:2], y[:2], th, MT.MARGINAL, b0, lam, X)["status"] == -1   # the n > 2 guard


def test_cases_cover_the_shapes_and_conditions():
    ns, Ds, Qs = set(), set(), set()
    absent_pos = flat_present = shuffled = False
    for cid, p in MT.patients():
        c = MT.case(cid)
        m, t, y = c["pts"][p]
        n, nd = t.shape[0], MT.nout(c["kidx"], c["D"])
        ns.add(n); Ds.add(nd); Qs.add(c["Q"])
        cnt = np.bincount(MT._meta(c["kidx"], m, n), minlength=nd)
        absent_pos |= bool(np.any((cnt == 0) & (c["lam"][p] > 0)))
        flat_present |= bool(np.any((cnt > 0) & (c["lam"][p] == 0)))
        assert not MT.improper(c["kidx"], c["D"], m, n, MT.MARGINAL, c["lam"][p])
        if m is not None:
            shuffled |= bool(np.any(np.diff(m) < 0))
    assert {3, 63, 64, 65, 130} <= ns and {1, 3, 24, 33, 64} <= Ds and {5, 9} <= Qs
    assert absent_pos and flat_present and shuffled


def test_budget_factor_M_and_caps():
    """M_MEAN from the two fp64 CPU programs alone: every spread <= M / 4, the largest above M / 8 (so M is the SMALLEST such power of
    two), and every budget under its cap without clipping -- the sweep holds no case whose budget a cap would have to cut"""
    worst, where = {}, {}
    for cid, p in MT.patients():
        c = MT.case(cid)
        for mode in (MT.MARGINAL, MT.FIXED):
            for jr in (0, 1):
                r = MT.programs_of(c, p, mode, jr)
                if r["e"] is None:
                    continue
                for k, v in r["e"].items():
                    assert all(np.isfinite(v)), (cid, p, mode, jr, k, v)
                    assert T.budget(v, MT.M_MEAN) <= MT.cap_of(k), (cid, p, mode, jr, k, v)
                    s = T.spread(v)
                    if s > worst.get(k, 0):
                        worst[k], where[k] = s, (cid, p, mode, jr)
    for k in worst:
        print(f"MEAN-SPREAD {k:9s} {worst[k]:7.1f} at {where[k]}")
    top = max(worst.values())
    assert top <= MT.M_MEAN / 4 and top > MT.M_MEAN / 8, worst
    assert abs(top - MT.MEASURED_SPREAD) <= 0.05 * MT.MEASURED_SPREAD, (top, MT.MEASURED_SPREAD)


def test_reference_layout_helpers():
    from medgp_amd import baseline
    th, mm = np.arange(10.0).reshape(2, 5), np.array([[0.5, -1.0], [2.0, 3.0]])
    x = baseline.reference_theta(th, mm)
    assert x.shape == (2, 7) and np.all(x[:, :5] == th) and np.all(x[:, 5:] == mm)
    a, b = baseline.split_reference_theta(x, 2)
    assert np.all(a == th) and np.all(b == mm)
    assert np.all(baseline.split_reference_grad(th, mm) == x)
    b0, lam = baseline.standard_prior(3)
    assert np.all(b0 == 0) and np.all(lam == 1) and np.all(baseline.flat(3)[1] == 0)
    assert baseline.fixed([1.0, 2.0])["fixed"] is True
    lo, hi = baseline.interval(np.array([1.0]), np.array([4.0]))
    assert abs(lo[0] - (1 - 2 * 1.959963984540054)) <= 1e-12 and abs(hi[0] - (1 + 2 * 1.959963984540054)) <= 1e-12


def test_mean_tables_walk_clean_under_sanitizers():
    subprocess.check_call(["make", "-s", "-C", CSRC, "mean_tables_test"])
    out = subprocess.run([os.path.join(CSRC, "mean_tables_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mean_tables ok" in out.stdout
