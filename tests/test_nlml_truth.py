"""CPU tests of the extended-precision truth (tests/nlml_truth.py) and of the fp64 error budget the GPU sweeps
(tests/test_nlml_budget_gpu.py) hold the device to.

* the truth against a 50-digit mpmath evaluation (nlml from the formula, every gradient component by mpmath's numerical
  differentiation of that nlml: no gradient formula is shared) on tiny cases of the three families;
* the block-sum form of the LMC gradient against tr(W dK/dtheta_h) / 2 hyper by hyper;
* translation invariance: the truth is bit-identical when every time stamp moves by an exactly representable offset;
* the errors of the three legitimate fp64 programs over every sweep case, the factor M they define, and the condition that no
  budget can hide a single-precision slip.
"""
import numpy as np
import pytest

import nlml_truth as T

# Agreement asked of the truth: 1e-15 in the error measures of the suite.  Long double carries eps = 1.1e-19; the tiny cases have
# cond(K) <= 1e3 and a few hundred operations per output, so 1e-15 is two decades of head room above what it should reach and three
# decades under the fp64 errors (1e-13 .. 1e-11) the truth is used to measure.  Reached: see test_truth_vs_mpmath's printout
# (worst 1.2e-18 nlml, 6.1e-16 gradient, both on the one-hour-period case).
MP_TOL = 1e-15

TINY = [
    # kidx, Q, D, R, n, seed, period range [h]
    (7, 2, 2, 1, 9, 1, (12.0, 72.0)),
    (7, 3, 3, 2, 12, 2, (1.0, 1.0)),       # one-hour period over a 200 h span: the large-angle regime
    (7, 1, 2, 2, 3, 3, (12.0, 72.0)),      # the smallest n the reference accepts
    (8, 1, 1, 0, 10, 4, None),
    (8, 3, 1, 0, 14, 5, None),
    (0, 1, 1, 0, 8, 6, None),
    (0, 1, 1, 0, 24, 7, None),
]


def _tiny_case(kidx, Q, D, R, n, seed, period):
    from medgp_amd import synth
    g = np.random.Generator(np.random.Philox(key=[777, seed]))
    t = np.sort(g.uniform(0.0, 200.0, size=n)).astype(np.float32)
    t[1] = t[0]                                            # a repeated time stamp
    m = np.sort(g.integers(0, D, size=n)).astype(np.int32) if kidx == 7 else None
    y = g.standard_normal(n).astype(np.float32)
    if kidx == 7:
        th = T._lmc_theta(g, Q, D, R, period=period, scale=(6.0, 72.0), noise=(0.15, 0.4))
    else:
        th = synth.theta(777, seed, kidx, Q, 1, 0)
    return m, t, y, th


def _mp_nlml(mp, kidx, Q, D, R, m, t, y, th):
    """nlml in mpmath arithmetic straight from the definition (th: list of mpf)"""
    n = len(t)
    pi = mp.mpf(float(T.REF_PI))
    tt = [mp.mpf(float(x)) for x in t]
    yy = mp.matrix([mp.mpf(float(x)) for x in y])
    K = mp.zeros(n, n)
    if kidx == 7:
        sig2 = [mp.exp(th[d]) ** 2 for d in range(D)]
        c = th[D:]
        A = [[[c[q * D * R + d * R + r] for r in range(R)] for d in range(D)] for q in range(Q)]
        mu = [mp.exp(c[Q * D * R + q]) for q in range(Q)]
        v = [mp.exp(c[Q * D * R + Q + q]) for q in range(Q)]
        kap = [[mp.exp(c[Q * (D * R + 2) + q * D + d]) for d in range(D)] for q in range(Q)]
        B = [[[sum(A[q][d][r] * A[q][e][r] for r in range(R)) + (kap[q][d] if d == e else 0) for e in range(D)] for d in range(D)]
             for q in range(Q)]
        for i in range(n):
            for j in range(n):
                dt = tt[i] - tt[j]
                K[i, j] = sum(B[q][int(m[i])][int(m[j])] * mp.cos(2 * pi * mu[q] * dt) * mp.exp(-2 * (pi * v[q]) ** 2 * dt ** 2)
                              for q in range(Q))
            K[i, i] += sig2[int(m[i])]
    elif kidx == 8:
        sig2 = mp.exp(th[0]) ** 2
        w = [mp.exp(th[1 + q]) for q in range(Q)]
        mu = [mp.exp(th[1 + Q + q]) for q in range(Q)]
        v = [mp.exp(th[1 + 2 * Q + q]) for q in range(Q)]
        for i in range(n):
            for j in range(n):
                dt = tt[i] - tt[j]
                K[i, j] = sum(w[q] * mp.cos(2 * pi * mu[q] * dt) * mp.exp(-2 * (pi * v[q]) ** 2 * dt ** 2) for q in range(Q))
            K[i, i] += sig2
    else:
        sig2, l, sf2 = mp.exp(th[0]) ** 2, mp.exp(th[1]), mp.exp(th[2]) ** 2
        for i in range(n):
            for j in range(n):
                K[i, j] = sf2 * mp.exp(-((tt[i] - tt[j]) / l) ** 2 / 2)
            K[i, i] += sig2
    L = mp.cholesky(K)
    alpha = mp.cholesky_solve(K, yy)
    quad = sum(yy[i] * alpha[i] for i in range(n))
    return quad / 2 + sum(mp.log(L[i, i]) for i in range(n)) + n * mp.log(2 * pi) / 2


@pytest.mark.parametrize("tiny", TINY, ids=lambda c: f"k{c[0]}_Q{c[1]}D{c[2]}R{c[3]}_n{c[4]}")
def test_truth_vs_mpmath(tiny):
    import mpmath
    mp = mpmath.mp
    kidx, Q, D, R, n, seed, period = tiny
    m, t, y, th = _tiny_case(kidx, Q, D, R, n, seed, period)
    st, nl, g = T.nlml_grad(kidx, Q, D, R, m, t, y, th)
    assert st == 0
    old = mp.dps
    mp.dps = 50
    try:
        thm = [mp.mpf(float(x)) for x in th]
        ref = _mp_nlml(mp, kidx, Q, D, R, m, t, y, thm)
        H = len(th)
        gref = []
        for h in range(H):
            def f(x, h=h):
                th2 = list(thm)
                th2[h] = x
                return _mp_nlml(mp, kidx, Q, D, R, m, t, y, th2)
            gref.append(mp.diff(f, thm[h]))
        en = float(abs(_to_mp(mp, nl) - ref) / abs(ref))      # compared in mpmath, then to float
        gs = max(abs(x) for x in gref)
        eg = max(float(abs(_to_mp(mp, g[h]) - gref[h]) / max(abs(gref[h]), gs / 1000)) for h in range(H))
    finally:
        mp.dps = old
    print(f"truth vs mpmath: nlml {en:.2e}, gradient {eg:.2e}")
    assert en <= MP_TOL and eg <= MP_TOL, (en, eg)


def _to_mp(mp, x):
    """exact conversion of a long double to mpf (hi + lo split into two doubles)"""
    x = np.longdouble(x)
    hi = np.float64(x)
    lo = np.float64(x - np.longdouble(hi))
    return mp.mpf(float(hi)) + mp.mpf(float(lo))


def test_block_sum_form_equals_per_hyper_trace():
    kidx, Q, D, R, n = 7, 3, 3, 2, 40
    m, t, y, th = _tiny_case(kidx, Q, D, R, n, 11, (12.0, 72.0))
    st, nl, g, (K, W, h) = T.nlml_grad(kidx, Q, D, R, m, t, y, th, want_parts=True)
    gn = T.lmc_grad_naive(Q, D, R, m, t, th, W)
    scale = np.maximum(np.abs(gn), 1e-3 * np.abs(gn).max())
    e = float(np.max(np.abs(g - gn) / scale))
    print(f"block-sum vs per-hyper trace: {e:.2e}")
    assert e <= 1e-16, e            # both in long double: they differ by summation order only (n^2 = 1600 terms of eps 1.1e-19)


def test_truth_is_translation_invariant_bit_for_bit():
    for case in T.time_cases():
        for off in T.TIME_OFFSETS[1:]:
            sh = T.shifted(case, off)
            for p in range(len(case["pts"])):
                a = T.truth_of(case, p)
                b = T.truth_of(sh, p)
                assert a[1] == b[1] and np.array_equal(a[2], b[2]), (case["id"], off, p)


def test_float64_run_is_the_same_code():
    """dtype=np.float64 returns doubles and stays within fp64 distance of the truth (it is program (b) of the budget)"""
    case = T.time_cases()[1]
    m, t, y = case["pts"][0]
    st, nl, g = T.nlml_grad(7, case["Q"], case["D"], case["R"], m, t, y, case["th"][0], np.float64)
    assert nl.dtype == np.float64 and g.dtype == np.float64
    _, tn, tg = T.truth_of(case, 0)
    en, eg = T.error_pair(nl, g, tn, tg)
    assert 0 < eg < 1e-10 and en < 1e-12


def test_guard_and_jitter_argument():
    m, t, y, th = _tiny_case(7, 2, 2, 1, 9, 1, (12.0, 72.0))
    assert T.nlml_grad(7, 2, 2, 1, m[:2], t[:2], y[:2], th)[0] == -1          # n > 2 guard
    K0 = T.gram(7, 2, 2, 1, m, t, th)
    K2 = T.gram(7, 2, 2, 1, m, t, th, jitter_rounds=2)
    sig2 = np.exp(np.asarray(th[:2], np.longdouble)) ** 2
    assert np.allclose(np.diagonal(K2 - K0).astype(np.float64), 2 * sig2[m].astype(np.float64), rtol=1e-15)
    assert T.nlml_grad(7, 2, 2, 1, m, t, y, th, jitter_rounds=2)[0] == 2


def _all_rows():
    rows = []
    for case in T.all_cases():
        for p in range(len(case["pts"])):
            r = T.programs_of(case, p)
            rows.append((case, p, r))
    return rows


def test_budget_factor_M_and_caps():
    """Over every case of every sweep: the errors of (a) the oracle, (b) the float64 run of the truth code, (c) the float64 run with
    cosine tables and blocked factorisation; M from their spread; every budget under its cap.  CPU programs only."""
    rows = _all_rows()
    per = {}
    worst_sn = worst_sg = 1.0
    for case, p, r in rows:
        assert r["status"] == 0, (case["id"], p, r["status"])      # no case of the sweeps sits in the jitter regime
        sn, sg = T.spread(r["en"]), T.spread(r["eg"])
        worst_sn, worst_sg = max(worst_sn, sn), max(worst_sg, sg)
        d = per.setdefault(case["sweep"], dict(en=0.0, eg=0.0, bn=0.0, bg=0.0, n=0))
        d["en"], d["eg"] = max(d["en"], max(r["en"])), max(d["eg"], max(r["eg"]))
        d["bn"], d["bg"] = max(d["bn"], T.budget(r["en"], T.M_NLML)), max(d["bg"], T.budget(r["eg"], T.M_GRAD))
        d["n"] += 1
        assert T.budget(r["eg"], T.M_GRAD) < T.GRAD_BUDGET_CAP, (case["id"], p, r["eg"])
        assert T.budget(r["en"], T.M_NLML) < T.NLML_BUDGET_CAP, (case["id"], p, r["en"])

    def rule(s):      # smallest power of two M with s <= M / 4
        M = 1
        while s > M / 4:
            M *= 2
        return M
    for sw, d in per.items():
        print(f"{sw:8s} {d['n']:3d} patients: worst E_nlml {d['en']:.2e} E_grad {d['eg']:.2e}; largest budget nlml {d['bn']:.2e} grad {d['bg']:.2e}")
    print(f"spread between the programs: nlml {worst_sn:.1f}, gradient {worst_sg:.1f} -> M_NLML {rule(worst_sn)}, M_GRAD {rule(worst_sg)}")
    # <=, not ==: the spreads sit near a power-of-two threshold (57.8 against 64) and another libm for the long-double cosine or
    # another reduction order in the oracle may move them; the constants must cover what is measured
    assert rule(worst_sn) <= T.M_NLML and rule(worst_sg) <= T.M_GRAD


# ---- the large sweep (N = 512 .. 4096) and its committed truths ------------------------------------------------------------------------

def test_large_sweep_is_complete():
    """how much of the large sweep may be left out is a condition: every case of nlml_truth.LARGE_IDS is there, except the optional
    ones that nlml_truth.LARGE_ABSENT names (DESIGN.md section 3 says why), with the sizes the GPU tests rely on"""
    assert T.LARGE_ABSENT <= T.LARGE_OPTIONAL == {"large_config5"}
    cases = {c["id"]: c for c in T.large_cases()}
    assert set(cases) == set(T.LARGE_IDS) - T.LARGE_ABSENT
    assert all(c["sweep"] == "large" for c in cases.values())
    assert set(cases) <= {c["id"] for c in T.all_cases()}
    ns = {cid: [p[1].shape[0] for p in c["pts"]] for cid, c in cases.items()}
    assert ns["large_headline"] == [512] * 8 and ns["large_pass2"] == [513, 576, 768, 1024]
    assert all(ns[f"large_q_Q{Q}"] == [640] and cases[f"large_q_Q{Q}"]["Q"] == Q for Q in (8, 9, 16, 17))
    assert ns["large_config3"] == [2048] and ns["large_slices"] == [2880] and ns["large_sm_Q4"] == [1024] and ns["large_se"] == [1024]
    assert (cases["large_headline"]["D"], cases["large_headline"]["Q"], cases["large_headline"]["R"]) == (24, 5, 8)
    assert (cases["large_config3"]["D"], cases["large_config3"]["Q"], cases["large_config3"]["R"]) == (24, 5, 8)
    if "large_config5" in cases:
        assert ns["large_config5"] == [4096] and cases["large_config5"]["D"] == 64
    hp = cases["large_headline"]["pts"]
    assert len({T.input_sha256(cases["large_headline"], p) for p in range(8)}) == 8            # eight DISTINCT patients
    assert any(len(np.unique(m)) < 24 for m, t, y in hp) and any(np.any(np.diff(m) < 0) for m, t, y in hp)      # missing, shuffled
    # the redraw rule replaces draws, it does not drop patients: every large id in DRAWS names patients that exist
    for cid, d in T.DRAWS.items():
        if cid.startswith("large_"):
            assert cid in cases and all(0 <= p < len(cases[cid]["pts"]) and 0 < k < 8 for p, k in d.items()), (cid, d)
    want = {f"{c['id']}:{p}" for c in cases.values() for p in range(len(c["pts"])) if c["pts"][p][1].shape[0] > T.FIXTURE_ABOVE_N}
    want.add("%s:%d" % T.FIXTURE_BIT_CHECK)
    assert {f"{c['id']}:{p}" for c, p in T.fixture_patients()} == want
    with np.load(T.LARGE_FIXTURE) as z:
        assert {str(x) for x in z["ids"]} == want             # and the fixture holds exactly these


def test_large_fixture_reproduces():
    """The committed truths are not trusted blind.  For every committed patient: the input hash matches, and program (a) (the
    oracle) and program (b) (the truth code in float64), recomputed here, have the stored errors against the stored truth to a factor
    of 2 (they are deterministic; the factor absorbs libm differences between machines).  A stored truth that was wrong by more than
    an fp64 rounding error would move both.  The n = 4096, D = 64 patient is left to the hash, status and shape checks: its two
    programs take 100 s here, which would put the CPU suite's growth over the three minutes it was given (measured: 35 s for the
    patients of n = 1024, 2048, 2880 together)."""
    checked = 0
    for case, p in T.fixture_patients():
        e = T.fixture_entry(case, p)                          # (raises on a missing entry or another input hash)
        assert e["status"] == 0, (case["id"], p)
        tn, tg = e["truth"]
        assert tg.shape == (T.num_hyp(case["kidx"], case["Q"], case["D"], case["R"]),)
        assert np.all(np.isfinite(tg.astype(np.float64))) and np.isfinite(float(tn))
        if case["pts"][p][1].shape[0] > 2880:
            continue
        checked += 1
        a = T.oracle_program(case, p)
        assert a["status"] == e["status"]
        _, bn, bg = T.float64_program(case, p, e["status"])
        for name, i, (en, eg) in (("a", 0, T.error_pair(a["nlml"], a["grad"], tn, tg)), ("b", 1, T.error_pair(bn, bg, tn, tg))):
            print(f"{case['id']}:{p} program ({name}): nlml {en:.3e} (stored {e['en'][i]:.3e}), gradient {eg:.3e} (stored {e['eg'][i]:.3e})")
            assert e["en"][i] / 2 <= en <= 2 * e["en"][i], (case["id"], p, name, en, e["en"][i])
            assert e["eg"][i] / 2 <= eg <= 2 * e["eg"][i], (case["id"], p, name, eg, e["eg"][i])
    assert checked == 3          # n = 1024, 2048, 2880


def test_large_fixture_truth_bits():
    """the one committed patient that is cheap enough (D = 3, n = 1024): its long-double truth recomputed here equals hi + lo bit for
    bit, and is the truth the run-time path uses for it"""
    cid, p = T.FIXTURE_BIT_CHECK
    case = [c for c in T.large_cases() if c["id"] == cid][0]
    assert case["pts"][p][1].shape[0] == 1024 and not T.in_fixture(case, p)
    e = T.fixture_entry(case, p)
    st, tn, tg = T.truth_of(case, p, e["status"])
    assert st == e["status"] and tn == e["truth"][0] and np.array_equal(tg, e["truth"][1])
    assert tn.dtype == np.longdouble and tg.dtype == np.longdouble


def test_large_fixture_fails_loudly_on_other_inputs():
    """a committed truth is bound to the bytes it was computed from: one changed observation and truth_of / programs_of raise"""
    case = [c for c in T.large_cases() if c["id"] == "large_config3"][0]
    assert T.in_fixture(case, 0)
    m, t, y = case["pts"][0]
    y2 = y.copy()
    y2[17] = np.nextafter(y2[17], np.float32(9))
    other = dict(case, pts=[(m, t, y2)])
    with pytest.raises(RuntimeError, match="other inputs"):
        T.programs_of(other, 0)
    other = dict(case, id="large_nowhere")
    with pytest.raises(RuntimeError, match="holds no truth"):
        T.truth_of(other, 0)
