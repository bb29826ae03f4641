"""CPU checks of tests/basis_truth.py, the definition medgp_basis_nlml_grad / medgp_basis_posterior_batch are held to: its Woodbury form
agrees with the dense form, its gradients are the derivatives of its own nlml, on the indicator basis it is mean_truth, its limits
hold, the budget factor is what the CPU programs measure, and the host-side geometry of the calls (basis_tables.h) walks clean under
sanitizers.  No GPU."""
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import basis_truth as BT   # noqa: E402
import mean_truth as MT    # noqa: E402
import nlml_truth as T     # noqa: E402
from test_mean_truth import _rel, _richardson, _small   # noqa: E402

X = np.longdouble
EPS = float(np.finfo(X).eps)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "medgp_amd", "csrc")


def _basis(kidx, m, t, p_extra=2, seed=3):
    """a trend basis with a step and random columns on a small patient: [n, 2 D + 1 + p_extra], well conditioned"""
    from medgp_amd import basis as B
    D = 3 if kidx == 7 else 1
    H = B.Design([B.intercept(D), B.linear(D, 100.0, 60.0), B.step(40.0, 150.0)]).design(m, t)
    g = T._philox(20261811, seed)
    return np.concatenate([H, g.standard_normal((H.shape[0], p_extra))], axis=1)


def _prior(p, seed=4):
    g = T._philox(20261812, seed)
    return 0.5 * g.standard_normal(p), g.uniform(0.05, 3.0, p)


def test_woodbury_equals_dense_gram():
    """all lam_c > 0: nlml, W~, alpha~ and the posterior of the Woodbury form are those of the zero-mean GP on K~ = K + H Lambda^-1 H^T"""
    for kidx in (7, 8, 0):
        fam, m, t, y, th, _, _ = _small(kidx)
        H = _basis(kidx, m, t)
        b0, lam = _prior(H.shape[1])
        for jr in (0, 2):
            w = BT.woodbury(*fam, m, t, y, th, H, BT.MARGINAL, b0, lam, X, jr, want_parts=True)
            d = BT.dense(*fam, m, t, y, th, H, b0, lam, X, jr)
            assert abs(w["nlml"] - d["nlml"]) <= 1e-15 * abs(d["nlml"])
            assert _rel(w["parts"]["W"], d["W"]) <= 1e-13 and _rel(w["parts"]["alpha_t"], d["alpha_t"]) <= 1e-13
            a, c = w["parts"]["quad_def"]
            assert abs(w["parts"]["quad"] - (a - c)) <= 64 * EPS * (abs(a) + abs(c))
            g = T._philox(20261813, kidx)
            m2 = g.integers(0, fam[2], 9).astype(np.int32) if kidx == 7 else None
            t2 = g.uniform(-20, 220, 9).astype(np.float32)
            h2 = g.standard_normal((9, H.shape[1]))
            p = BT.posterior(*fam, m, t, y, th, H, BT.MARGINAL, b0, lam, m2, t2, h2, X, jr)
            dm, dv = BT.dense_posterior(*fam, m, t, y, th, H, b0, lam, m2, t2, h2, X, jr)
            assert _rel(p["mean"], dm) <= 1e-13 and _rel(p["var"], dv) <= 1e-13
            assert np.all(p["extra"] >= 0) and np.all(p["var"] >= p["var0"])


def test_gradients_are_the_derivatives_of_the_truths_own_nlml():
    """Richardson differences in theta, b0 and log lam"""
    from medgp_amd import basis as B
    for kidx, mode in ((7, BT.MARGINAL), (7, BT.FIXED), (8, BT.MARGINAL), (0, BT.MARGINAL)):
        fam, m, t, y, th, _, _ = _small(kidx, n=24)
        H = _basis(kidx, m, t, p_extra=1)
        p = H.shape[1]
        b0, lam = _prior(p)
        lam0 = lam.copy()
        lam0[0] = 0.0   # one flat column
        r = BT.woodbury(*fam, m, t, y, th, H, mode, b0, lam0, X)
        f = lambda x: BT.woodbury(*fam, m, t, y, x, H, mode, b0, lam0, X, want_grad=False)["nlml"]   # noqa: E731
        scale = float(np.abs(r["grad"]).max())
        for i in range(th.shape[0]):
            d, bound = _richardson(f, th, i, 2.0 ** -20)
            assert bound <= 1e-9 * scale, (kidx, mode, i, float(bound), scale)   # the check has teeth
            assert abs(d - r["grad"][i]) <= bound + 1e-15 * scale, (kidx, mode, i, float(d), float(r["grad"][i]), float(bound))
        fb = lambda x: BT.woodbury(*fam, m, t, y, th, H, mode, x, lam0, X, want_grad=False)["nlml"]   # noqa: E731
        for c in range(p):
            v, bound = _richardson(fb, b0, c, 2.0 ** -10)
            assert abs(v - r["dbeta"][c]) <= bound + 1e-14 * float(np.abs(r["dbeta"]).max() + 1e-300), (kidx, mode, c)
        # dbeta = -H^T alpha~ in both modes
        rp = BT.woodbury(*fam, m, t, y, th, H, mode, b0, lam0, X, want_grad=False, want_parts=True)
        assert np.abs(rp["dbeta"] + rp["parts"]["Hm"].T @ rp["parts"]["alpha_t"]).max() <= 1e-15 * float(rp["dbeta_mag"].max())
        if mode == BT.MARGINAL:
            r1 = BT.woodbury(*fam, m, t, y, th, H, mode, b0, lam, X, want_grad=False)
            db, dl = MT.prior_grad(r1["beta"], r1["beta_cov"], b0, lam)
            assert np.all(db == r1["dbeta"])
            fl = lambda x: BT.woodbury(*fam, m, t, y, th, H, mode, b0, np.exp(x), X, want_grad=False)["nlml"]   # noqa: E731
            for c in range(p):
                v, bound = _richardson(fl, np.log(lam), c, 2.0 ** -10)
                assert abs(v - dl[c]) <= bound + 1e-12 * float(np.abs(dl).max()), (c, float(v), float(dl[c]), float(bound))
            hb, hl = B.prior_grad(r1["beta"].astype(np.float64), r1["beta_cov"].astype(np.float64), b0, lam)
            assert _rel(hb, db) <= 1e-14 and _rel(hl, dl) <= 1e-13


def test_indicator_basis_is_the_baseline_truth():
    """H = mean_truth.hmat: every output equals mean_truth.woodbury's to long-double rounding, both modes, also the posterior"""
    for kidx in (7, 8, 0):
        fam, m, t, y, th, b0, lam = _small(kidx)
        n = t.shape[0]
        H = MT.hmat(kidx, fam[2], m, n, np.float64)
        g = T._philox(20261814, kidx)
        m2 = g.integers(0, fam[2], 7).astype(np.int32) if kidx == 7 else None
        t2 = g.uniform(-20, 220, 7).astype(np.float32)
        h2 = MT.hmat(kidx, fam[2], m2, 7, np.float64)
        for mode in (BT.MARGINAL, BT.FIXED):
            lm = lam.copy()
            if mode == BT.MARGINAL:
                lm[0] = 0.0
            a = BT.woodbury(*fam, m, t, y, th, H, mode, b0, lm, X, 1)
            b = MT.woodbury(*fam, m, t, y, th, mode, b0, lm, X, 1)
            assert a["status"] == b["status"] == 1
            assert abs(a["nlml"] - b["nlml"]) <= 4 * EPS * abs(b["nlml"]) and _rel(a["grad"], b["grad"]) <= 1e-16
            assert _rel(a["dbeta"], b["dmean"]) <= 1e-16 and _rel(a["beta"], b["beta"]) <= 1e-16 and np.abs(a["beta_cov"] - b["beta_cov"]).max() <= 1e-17
            assert _rel(a["dbeta_mag"], b["dmean_mag"]) <= 1e-16
            pa = BT.posterior(*fam, m, t, y, th, H, mode, b0, lm, m2, t2, h2, X)
            pb = MT.posterior(*fam, m, t, y, th, mode, b0, lm, m2, t2, X)
            assert _rel(pa["mean"], pb["mean"]) <= 1e-16 and _rel(pa["var"], pb["var"]) <= 1e-16


def test_fixed_at_zero_is_the_plain_nlml():
    for kidx in (7, 8, 0):
        fam, m, t, y, th, _, _ = _small(kidx)
        H = _basis(kidx, m, t)
        for jr in (0, 1):
            r = BT.woodbury(*fam, m, t, y, th, H, BT.FIXED, np.zeros(H.shape[1]), None, X, jr)
            st, nl, g = T.nlml_grad(*fam, m, t, y, th, X, jr)
            assert r["status"] == st == jr
            assert abs(r["nlml"] - nl) <= 1e-17 * abs(nl) and _rel(r["grad"], g) <= 1e-15
            assert np.all(r["beta"] == 0) and np.all(r["beta_cov"] == 0)


def test_dependent_flat_columns_are_improper_and_a_zero_column_is_legal():
    fam, m, t, y, th, _, _ = _small(7)
    H = _basis(7, m, t)
    p = H.shape[1]
    b0, lam = _prior(p + 1)
    Hd = np.concatenate([H, H[:, :1]], axis=1)        # the last column repeats the first
    lam_flat = lam.copy()
    lam_flat[[0, p]] = 0.0
    for dt in (X, np.float64):
        assert BT.woodbury(*fam, m, t, y, th, Hd, BT.MARGINAL, b0, lam_flat, dt)["status"] == -1
    assert BT.posterior(*fam, m, t, y, th, Hd, BT.MARGINAL, b0, lam_flat, m[:2], t[:2], Hd[:2], X)["status"] == -1
    assert BT.woodbury(*fam, m, t, y, th, Hd, BT.MARGINAL, b0, lam, X)["status"] == 0        # proper under lam > 0
    assert BT.woodbury(*fam, m, t, y, th, Hd, BT.FIXED, b0, None, X)["status"] == 0          # FIXED ignores lam
    assert BT.woodbury(*fam, m[:2], t[:2], y[:2], th, Hd[:2], BT.MARGINAL, b0, lam, X)["status"] == -1   # the n > 2 guard
    # a zero column with lam_c > 0: beta^_c = b0_c, A^-1 has 1 / lam_c there, and the variance at a point gains h*^2 / lam_c
    Hz = np.concatenate([H, np.zeros((H.shape[0], 1))], axis=1)
    r = BT.woodbury(*fam, m, t, y, th, Hz, BT.MARGINAL, b0, lam, X)
    assert r["status"] == 0 and r["beta"][p] == X(b0[p]) and r["dbeta"][p] == 0
    e = np.zeros(p + 1, X)
    e[p] = 1 / X(lam[p])
    assert np.abs(r["beta_cov"][p] - e).max() <= 1e-18
    h2 = np.concatenate([Hz[:1, :p], [[3.0]]], axis=1)
    h0 = np.concatenate([Hz[:1, :p], [[0.0]]], axis=1)
    pa = BT.posterior(*fam, m, t, y, th, Hz, BT.MARGINAL, b0, lam, m[:1], t[:1] + 0.5, h2, X)
    pb = BT.posterior(*fam, m, t, y, th, Hz, BT.MARGINAL, b0, lam, m[:1], t[:1] + 0.5, h0, X)
    assert abs((pa["var"][0] - pb["var"][0]) - 9 / X(lam[p])) <= 1e-16 * float(pa["var"][0])


def test_cases_cover_the_shapes_and_conditions():
    from medgp_amd import basis as B
    ns, ps, fams = set(), set(), set()
    flat = shuffled = False
    for cid, q in BT.patients():
        c = BT.case(cid)
        m, t, y = c["pts"][q]
        ns.add(t.shape[0]); ps.add(c["p"]); fams.add((c["kidx"], c["D"]))
        assert c["H"][q].shape == (t.shape[0], c["p"]) and c["Q"] <= 16
        flat |= bool(np.any(c["lam"][q] == 0))
        assert set(c["lam"][q]) <= set(BT.LAM_CHOICES)
        if np.any(c["lam"][q] == 0):
            assert B.conditioning(c["H"][q]) <= BT.COND_FLAT
        if m is not None:
            shuffled |= bool(np.any(np.diff(m) < 0))
        if c["kind"] == "step":   # a strict sub-interval
            assert 0 < c["H"][q].sum() < t.shape[0]
    assert {3, 17, 63, 64, 65, 130, 200} <= ns and {1, 2, 16, 17, 33, 64} <= ps and {(0, 1), (8, 1), (7, 3), (7, 24)} <= fams
    assert flat and shuffled and len(BT.patients()) <= 16


def test_budget_factor_M_and_caps():
    """M_BASIS from the two fp64 CPU programs alone: every spread <= M / 4, the largest above M / 8 (so M is the SMALLEST such power of
    two), and every budget under its cap without clipping"""
    worst, where = {}, {}
    for cid, q in BT.patients():
        c = BT.case(cid)
        for mode in (BT.MARGINAL, BT.FIXED):
            for jr in (0, 1):
                r = BT.programs_of(c, q, mode, jr)
                assert r["e"] is not None, (cid, q, mode, jr)
                for k, v in r["e"].items():
                    assert all(np.isfinite(v)), (cid, q, mode, jr, k, v)
                    assert T.budget(v, BT.M_BASIS) <= BT.cap_of(k), (cid, q, mode, jr, k, v)
                    s = T.spread(v)
                    if s > worst.get(k, 0):
                        worst[k], where[k] = s, (cid, q, mode, jr)
    for k in worst:
        print(f"BASIS-SPREAD {k:9s} {worst[k]:7.1f} at {where[k]}")
    top = max(worst.values())
    assert top <= BT.M_BASIS / 4 and top > BT.M_BASIS / 8, worst
    assert abs(top - BT.MEASURED_SPREAD) <= 0.05 * BT.MEASURED_SPREAD, (top, BT.MEASURED_SPREAD)


def test_basis_tables_walk_clean_under_sanitizers():
    subprocess.check_call(["make", "-s", "-C", CSRC, "basis_tables_test"])
    out = subprocess.run([os.path.join(CSRC, "basis_tables_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "basis_tables ok" in out.stdout
