"""medgp_forecast_batch on the MI355X: every point against a REFIT of its prefix (forecast_ref.refit) on the cases of
forecast_cases.py -- all families, separable / generic kernels, caller-order and grouped uploads, several size classes, route
pinned and not -- the prior, prefix == NULL, monotonicity in the prefix, bit invariance of a point's outputs, jitter rounds,
failed patients, an asynchronous gradient lane in flight, no state left behind for medgp_posterior_batch, and one end-to-end
rolling-origin score."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
from medgp_amd import forecast, synth
import forecast_cases as FC
import forecast_ref as FR


def make_ctx(fam, pts, nbatch=None):
    ctx = medgp_amd.Context(*fam)
    ctx.reserve(len(pts), max(max(p[1].shape[0] for p in pts), 1), nbatch or len(pts))
    for s, (m, t, y) in enumerate(pts):
        ctx.set_patient(s, m if fam[0] == 7 else None, t, y)
    return ctx


def check_case(i, out, st, jitter_rounds=0, sel=None):
    fam, pts, th, qs = FC.case_data(i)
    sel = list(range(len(pts))) if sel is None else sel
    assert np.all(st == jitter_rounds), st
    worst = np.zeros(3)
    for k, p in enumerate(sel):
        m2, t2, y2, pf = qs[p]
        worst = np.maximum(worst, FR.check_forecast(fam[0], fam[2], th[p], m2 if fam[0] == 7 else None, pf, FC.case_ref(i, p, jitter_rounds), out[k]))
    print(f"case {i} ({FC.case_id(FC.CASES[i])}) jitter {jitter_rounds}: worst mean {worst[0]:.3f} / var {worst[1]:.3f} fp32 ulps, "
          f"lpd {worst[2]:.3g} (bound {FR.lpd_bound():.3g})")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("i", range(len(FC.CASES)), ids=[FC.case_id(s) for s in FC.CASES])
def test_every_point_matches_a_refit_of_its_prefix(i):
    fam, pts, th, qs = FC.case_data(i)
    ctx = make_ctx(fam, pts)
    out, st = ctx.forecast(np.arange(len(pts)), th, *FC.call_lists(fam, qs))
    if i == 0:
        assert len(ctx.last_plan()) >= 3, ctx.last_plan()   # the multi-class call
    check_case(i, out, st)
    # the prior, explicitly: var == float32(k** + sigma^2) to the bar is part of check_forecast (the refit of prefix 0 is the
    # Gram diagonal of the points); here the mean and the lpd-less call
    out2, st2 = ctx.forecast(np.arange(len(pts)), th, *FC.call_lists(fam, qs)[:3])
    for a, b in zip(out, out2):
        assert b[2] is None and same_bits(a[:2], b[:2])
    ctx.close()


def test_route_pinned():
    fam, pts, th, qs = FC.case_data(0)
    ctx = make_ctx(fam, pts)
    ctx.pin_route(True)
    out, st = ctx.forecast(np.arange(len(pts)), th, *FC.call_lists(fam, qs))
    assert {r for (_, _, r) in ctx.last_plan()} == {1}
    check_case(0, out, st)
    ctx.close()


def test_prefix_null_is_prefix_n_bit_for_bit():
    fam, pts, th, qs = FC.case_data(0)
    sel = [0, 1, 2, 5]   # caller-order copies and a grouped upload
    ctx = make_ctx(fam, [pts[p] for p in sel])
    m2l, t2l, _, y2l = FC.call_lists(fam, qs, sel)
    full = [np.full(qs[p][1].shape[0], pts[p][1].shape[0], np.int32) for p in sel]
    a, sa = ctx.forecast(np.arange(len(sel)), th[sel], m2l, t2l, None, y2l)
    b, sb = ctx.forecast(np.arange(len(sel)), th[sel], m2l, t2l, full, y2l)
    assert np.all(sa == 0) and np.all(sb == 0)
    for x, y in zip(a, b):
        assert same_bits(x, y)
    # and it is the posterior of all the data
    for k, p in enumerate(sel):
        ref = FR.refit(*FC.fam_args(fam, pts[p]), th[p], qs[p][0], qs[p][1], full[k], qs[p][2])
        FR.check_forecast(fam[0], fam[2], th[p], qs[p][0], full[k], ref, a[k])
    ctx.close()


def test_full_prefix_is_the_posterior_bit_for_bit():
    """k_forecast and k_posterior run the same panel-solve functions (kernels_posterior.h), so on the same factor a column with
    the full prefix goes through k_posterior's instructions: mean and var are equal as bits.  k_forecast works on the
    caller-order copy, which is the internal order only for a grouped upload or D = 1: those patients, over one, two and five
    panels, the separable and the generic K* form."""
    for i, sel in ((0, [1, 3]), (1, [2]), (3, [1]), (5, [0, 1]), (2, [0])):
        fam, pts, th, qs = FC.case_data(i)
        assert all(fam[2] == 1 or np.all(np.diff(pts[p][0]) >= 0) for p in sel)   # the caller's order is the internal order
        ctx = make_ctx(fam, [pts[p] for p in sel])
        m2l, t2l, _, _ = FC.call_lists(fam, qs, sel)
        f, sf = ctx.forecast(np.arange(len(sel)), th[sel], m2l, t2l)
        a, sa = ctx.posterior(np.arange(len(sel)), th[sel], m2l, t2l, parts=False)
        b, sb = ctx.posterior(np.arange(len(sel)), th[sel], m2l, t2l, parts=True)
        ctx.close()
        assert np.all(sf == 0) and np.all(sa == 0) and np.all(sb == 0)
        for k, p in enumerate(sel):
            assert f[k][0].shape == (qs[p][1].shape[0],)
            assert same_bits(f[k][:2], a[k][:2]) and same_bits(f[k][:2], b[k][:2]), (i, p)


@pytest.mark.parametrize("i,p", [(0, 0), (5, 0)])
def test_var_is_monotone_in_the_prefix(i, p):
    """q only ever gains non-negative terms, in a fixed order: exactly non-increasing, across tiles and panel counts"""
    fam, pts, th, qs = FC.case_data(i)
    n = pts[p][1].shape[0]
    ctx = make_ctx(fam, [pts[p]])
    pf = np.arange(n + 1, dtype=np.int32)
    g = np.random.default_rng(3)
    order = g.permutation(n + 1)
    for j in (0, 7):
        m2 = np.full(n + 1, qs[p][0][j], np.int32)
        t2 = np.full(n + 1, qs[p][1][j], np.float32)
        out, st = ctx.forecast([0], th[p][None, :], [m2] if fam[0] == 7 else None, [t2], [pf[order]])
        var = np.empty(n + 1, np.float32)
        var[order] = out[0][1]
        assert st[0] == 0 and np.all(np.diff(var.astype(np.float64)) <= 0.0)
        assert var[0] > var[n]
    ctx.close()


def test_point_outputs_are_bit_invariant(monkeypatch):
    fam, pts, th, qs = FC.case_data(0)
    P = len(pts)
    ctx = make_ctx(fam, pts)
    ctx.pin_route(True)
    ref, st = ctx.forecast(np.arange(P), th, *FC.call_lists(fam, qs))
    assert np.all(st == 0)
    # shuffled positions
    g = np.random.default_rng(1)
    perm = [g.permutation(q[1].shape[0]) for q in qs]
    sh, _ = ctx.forecast(np.arange(P), th, *[[a[perm[p]] for p, a in enumerate(lst)] for lst in FC.call_lists(fam, qs)])
    for p in range(P):
        assert same_bits(sh[p], [a[perm[p]] for a in ref[p]]), p
    # other points added in front and behind (other tiles, other panel counts), and a few points alone
    ex = [FC.points(g, fam[2], pts[p][1], 37) + (g.integers(0, pts[p][1].shape[0] + 1, size=37).astype(np.int32),) for p in range(P)]
    m2l, t2l, pfl, y2l = FC.call_lists(fam, qs)
    cat = lambda k, lst: [np.concatenate([ex[p][k][:20], lst[p], ex[p][k][20:]]) for p in range(P)]
    ad, _ = ctx.forecast(np.arange(P), th, cat(0, m2l), cat(1, t2l), cat(3, pfl), cat(2, y2l))
    for p in range(P):
        assert same_bits([a[20:20 + qs[p][1].shape[0]] for a in ad[p]], ref[p]), p
    for p, j in ((0, 0), (0, 199), (1, 64), (5, 3)):
        one, _ = ctx.forecast([p], th[p][None, :], [m2l[p][j:j + 1]], [t2l[p][j:j + 1]], [pfl[p][j:j + 1]], [y2l[p][j:j + 1]])
        assert same_bits(one[0], [a[j:j + 1] for a in ref[p]]), (p, j)
    # other batch-mates (route pinned)
    sel = [5, 0, 2]
    bm, _ = ctx.forecast(sel, th[sel], *FC.call_lists(fam, qs, sel))
    for k, p in enumerate(sel):
        assert same_bits(bm[k], ref[p]), p
    ctx.close()
    # a work budget of one tile per launch chunk
    monkeypatch.setenv("MEDGP_POSTERIOR_BUDGET_GB", "1e-6")
    ctx = make_ctx(fam, pts)
    ctx.pin_route(True)
    ctx.profile_enable(True, only="k_forecast")
    ch, _ = ctx.forecast(np.arange(P), th, *FC.call_lists(fam, qs))
    assert ctx.profile_read()["k_forecast"][1] == sum((q[1].shape[0] + 63) // 64 for q in qs)   # one launch per tile
    for p in range(P):
        assert same_bits(ch[p], ref[p]), p
    ctx.close()


@pytest.mark.parametrize("rounds", [1, 2])
def test_jitter_rounds(monkeypatch, rounds):
    monkeypatch.setenv("MEDGP_DEBUG_FAIL_ATTEMPTS", str(rounds))
    i = 1
    fam, pts, th, qs = FC.case_data(i)
    ctx = make_ctx(fam, pts)
    out, st = ctx.forecast(np.arange(len(pts)), th, *FC.call_lists(fam, qs))
    check_case(i, out, st, jitter_rounds=rounds)
    ctx.close()


def _singular(D):
    return (np.zeros(6, np.int32), np.array([1, 1, 1, 2, 2, 2], np.float32), np.ones(6, np.float32))


def test_failed_patient_gives_nan_and_spares_the_others():
    i = 1
    fam, pts, th, qs = FC.case_data(i)
    pts2 = [pts[0], _singular(fam[2]), pts[1], pts[2]]
    th2 = np.stack([th[0], th[0], th[1], th[2]])
    th2[1, :fam[2]] = -80.0   # no noise: the reference's jitter loop gives up (status -1)
    bad = (np.zeros(5, np.int32), np.linspace(0, 3, 5).astype(np.float32), np.zeros(5, np.float32), np.array([0, 1, 3, 6, 6], np.int32))
    qs2 = [qs[0], bad, qs[1], qs[2]]
    ctx = make_ctx(fam, pts2)
    out, st = ctx.forecast(np.arange(4), th2, *FC.call_lists(fam, qs2))
    assert st[1] < 0 and st[0] == 0 and st[2] == 0 and st[3] == 0
    assert all(np.all(np.isnan(a)) for a in out[1])
    check_case(i, [out[0], out[2], out[3]], st[[0, 2, 3]])
    ctx.close()


def test_async_gradient_lane_in_flight():
    i = 1
    fam, pts, th, qs = FC.case_data(i)
    P, H = len(pts), th.shape[1]
    ctx = make_ctx(fam, pts)
    nl_ref, gr_ref, st_ref = ctx.nlml_grad(np.arange(P), th, True)
    lane_th = ctx.pinned((P, H), np.float64); lane_th[:] = th
    lane_nl = ctx.pinned((P,), np.float64)
    lane_gr = ctx.pinned((P, H), np.float64)
    lane_st = ctx.pinned((P,), np.int32)
    ctx.nlml_grad_async(0, np.arange(P), lane_th, True, lane_nl, lane_gr, lane_st)
    out, st = ctx.forecast(np.arange(P), th, *FC.call_lists(fam, qs))
    ctx.wait(0)
    assert np.array_equal(lane_st, st_ref) and np.array_equal(lane_nl, nl_ref) and np.array_equal(lane_gr, gr_ref)
    check_case(i, out, st)
    ctx.close()


def test_posterior_bits_are_unchanged_by_a_forecast_call():
    fam, pts, th, qs = FC.case_data(0)
    P = len(pts)
    ctx = make_ctx(fam, pts)
    m2l, t2l, pfl, y2l = FC.call_lists(fam, qs)
    before, sb = ctx.posterior(np.arange(P), th, m2l, t2l)
    out, st = ctx.forecast(np.arange(P), th, m2l, t2l, pfl, y2l)
    after, sa = ctx.posterior(np.arange(P), th, m2l, t2l)
    assert np.array_equal(sb, sa) and np.all(st == 0)
    for a, b in zip(before, after):
        assert same_bits(a, b)
    check_case(0, out, st)
    ctx.close()


def test_argument_errors_and_capacity(monkeypatch):
    fam, pts, th, qs = FC.case_data(1)
    ctx = make_ctx(fam, pts)
    m2l, t2l, pfl, y2l = FC.call_lists(fam, qs)
    for badv in (-1, pts[1][1].shape[0] + 1):
        pf = [a.copy() for a in pfl]
        pf[1][3] = badv
        with pytest.raises(medgp_amd.MedgpError) as e:
            ctx.forecast(np.arange(3), th, m2l, t2l, pf, y2l)
        assert "prefix" in str(e.value) and "-1" in str(e.value)
    m2 = [a.copy() for a in m2l]
    m2[0][0] = fam[2]
    with pytest.raises(medgp_amd.MedgpError):
        ctx.forecast(np.arange(3), th, m2, t2l, pfl, y2l)
    # the context still works
    out, st = ctx.forecast(np.arange(3), th, m2l, t2l, pfl, y2l)
    check_case(1, out, st)
    ctx.close()
    monkeypatch.setenv("MEDGP_MEM_BUDGET_GB", "0.0001")   # 107 kB: the call cannot hold its matrices at once
    ctx = make_ctx(fam, pts)
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.forecast(np.arange(3), th, m2l, t2l, pfl, y2l)
    assert "memory budget" in str(e.value) and "-4" in str(e.value)
    ctx.close()


def test_rolling_origin_scores_end_to_end():
    """rolling_origin at horizons {0, 12} h on a 3-covariate patient of n = 150, uploaded in time order: the scores of the device's
    forecasts equal the scores of the refit reference to the float bar (coverage: the same points inside, except where a point
    sits within the bar of the interval's edge)."""
    fam = (7, 3, 3, 2)
    g = np.random.Generator(np.random.Philox(key=[FC.SEED, 99]))
    meta, t, y = FC.patient(g, 3, 150, "time")
    th = synth.theta(FC.SEED, 99, *fam)
    m2, t2, y2, pf, hi = forecast.rolling_origin(meta, t, y, [0.0, 12.0])
    assert np.any(pf == 0) and pf.max() >= 140
    ctx = make_ctx(fam, [(meta, t, y)])
    out, st = ctx.forecast([0], th[None, :], [m2], [t2], [pf], [y2])
    ctx.close()
    assert st[0] == 0
    ref = FR.refit(*fam, meta, t, y, th, m2, t2, pf, y2)
    FR.check_forecast(fam[0], fam[2], th, m2, pf, ref, out[0])
    sd = forecast.score(m2, y2, hi, *out[0], D=3, nh=2)
    sr = forecast.score(m2, y2, hi, *ref, D=3, nh=2)
    assert np.array_equal(sd["count"], sr["count"]) and sd["count"].sum() == 300
    # |mae_dev - mae_ref| <= mean |mean_dev - mean_ref| <= the bar at the patient's largest |mean|
    np.testing.assert_allclose(sd["mae"], sr["mae"], rtol=0, atol=2.0 ** -22 * np.abs(ref[0]).max())
    np.testing.assert_allclose(sd["lpd"], sr["lpd"], rtol=0, atol=FR.lpd_bound() * max(1.0, np.abs(ref[2]).max()))
    # a point changes sides only if |err| - 1.96 sd is within the float bar of 0
    edge = np.abs(np.abs(y2 - ref[0]) - forecast.CI95 * np.sqrt(ref[1])) <= 2.0 ** -20 * (np.abs(ref[0]).max() + np.sqrt(ref[1].max()))
    for d in range(3):
        for h in range(2):
            sel = (m2 == d) & (hi == h)
            assert abs(sd["coverage"][d, h] - sr["coverage"][d, h]) <= 100.0 * edge[sel].sum() / sel.sum()
