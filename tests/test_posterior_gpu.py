"""medgp_posterior_batch on the MI355X: parity with the numpy restatement of parsed_predict (posterior_ref.py) and with
medgp_fit_predict, every factorisation route and covariance family, ragged point counts, bit invariance of a point's
outputs, failed entries and the capacity error."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
from medgp_amd import synth
from posterior_ref import check_posterior, restate


def make_ctx(kidx, Q, D, R, pts):
    ctx = medgp_amd.Context(kidx, Q, D, R)
    ctx.reserve(len(pts), max(max(p[1].shape[0] for p in pts), 1), len(pts))
    for s, (m, t, y) in enumerate(pts):
        ctx.set_patient(s, m if kidx == 7 else None, t, y)
    return ctx


def grid(seed, D, t, m):
    """m test points: random covariates, times over the patient's range and a little beyond"""
    g = np.random.default_rng(seed)
    return (g.integers(0, D, size=m).astype(np.int32),
            g.uniform(float(t.min()) - 3.0, float(t.max()) + 3.0, size=m).astype(np.float32))


def check(kidx, Q, D, R, pt, th, m2, t2, mean, var, parts):
    """two fp32 ulps of the restatement per element, parts summing to the mean, var >= sigma^2 (posterior_ref.check_posterior)"""
    m, t, y = pt
    multi = kidx == 7
    ref = restate(kidx, Q, D, R, m if multi else None, t, y, th, m2 if multi else None, t2)
    check_posterior(kidx, D, th, m2 if multi else None, ref, mean, var, parts)


@pytest.mark.parametrize("D,Q,R,sizes,npts", [
    (3, 3, 2, (70, 131, 5, 200), (40, 70, 9, 1)),
    (24, 5, 8, (300, 97, 512), (130, 24, 64)),
])
def test_parity_with_restatement(D, Q, R, sizes, npts):
    pts = [synth.patient(21, p, D, n, interleave=True) for p, n in enumerate(sizes)]   # callers' order, not grouped
    th = np.stack([synth.theta(21, p, 7, Q, D, R) for p in range(len(pts))])
    gr = [grid(100 + p, D, pts[p][1], k) for p, k in enumerate(npts)]
    ctx = make_ctx(7, Q, D, R, pts)
    out, st = ctx.posterior(np.arange(len(pts)), th, [g[0] for g in gr], [g[1] for g in gr])
    assert np.all(st == 0)
    for p in range(len(pts)):
        check(7, Q, D, R, pts[p], th[p], gr[p][0], gr[p][1], *out[p])
    ctx.close()


def test_agrees_with_fit_predict():
    D, Q, R = 6, 4, 3
    pts = [synth.patient(33, 0, D, 260, interleave=True)]
    th = synth.theta(33, 0, 7, Q, D, R)
    m2, t2 = grid(5, D, pts[0][1], 150)
    ctx = make_ctx(7, Q, D, R, pts)
    out, st = ctx.posterior([0], th[None, :], [m2], [t2])
    fm, fv, fs = ctx.fit_predict(0, th, m2, t2)
    assert st[0] == 0 and fs == 0
    mean, var, _ = out[0]
    np.testing.assert_allclose(mean, fm, rtol=2e-6, atol=1e-6 * np.abs(fm).max())
    np.testing.assert_allclose(var, fv, rtol=2e-6, atol=1e-6 * np.abs(fv).max())
    ctx.close()


def test_routes_all_three_and_pinned():
    """One call whose size classes take the 4-wave (route 0), 8-wave (1) and look-ahead (2) factorisations."""
    D, Q, R = 2, 2, 2
    sizes = [1000] + [330] * 200 + [60] * 4
    pts = [synth.patient(44, p, D, n) for p, n in enumerate(sizes)]
    th = np.stack([synth.theta(44, p, 7, Q, D, R) for p in range(len(pts))])
    chk = [0, 1, 200, 201, 204]
    gr = [grid(200 + p, D, pts[p][1], 70 if p in chk else 0) for p in range(len(pts))]
    ctx = make_ctx(7, Q, D, R, pts)
    out, st = ctx.posterior(np.arange(len(pts)), th, [g[0] for g in gr], [g[1] for g in gr])
    routes = {r for (_, _, r) in ctx.last_plan()}
    assert routes == {0, 1, 2}, ctx.last_plan()
    assert np.all(st == 0)
    for p in chk:
        check(7, Q, D, R, pts[p], th[p], gr[p][0], gr[p][1], *out[p])
    ctx.pin_route(True)
    out2, st2 = ctx.posterior(chk, th[chk], [gr[p][0] for p in chk], [gr[p][1] for p in chk])
    assert {r for (_, _, r) in ctx.last_plan()} == {1}
    assert np.all(st2 == 0)
    for i, p in enumerate(chk):
        check(7, Q, D, R, pts[p], th[p], gr[p][0], gr[p][1], *out2[i])
    ctx.close()


def test_forced_multi_cu_route(monkeypatch):
    monkeypatch.setenv("MEDGP_MULTI_CU", "1")
    D, Q, R = 4, 3, 2
    pts = [synth.patient(45, p, D, n) for p, n in enumerate((140, 250))]
    th = np.stack([synth.theta(45, p, 7, Q, D, R) for p in range(2)])
    gr = [grid(300 + p, D, pts[p][1], 90) for p in range(2)]
    ctx = make_ctx(7, Q, D, R, pts)
    out, st = ctx.posterior([0, 1], th, [g[0] for g in gr], [g[1] for g in gr])
    assert {r for (_, _, r) in ctx.last_plan()} == {2}
    for p in range(2):
        check(7, Q, D, R, pts[p], th[p], gr[p][0], gr[p][1], *out[p])
    ctx.close()


def test_generic_component_count():
    D, Q, R = 2, 17, 1
    pts = [synth.patient(46, p, D, n) for p, n in enumerate((90, 150))]
    th = np.stack([synth.theta(46, p, 7, Q, D, R) for p in range(2)])
    gr = [grid(400 + p, D, pts[p][1], 50) for p in range(2)]
    ctx = make_ctx(7, Q, D, R, pts)
    out, st = ctx.posterior([0, 1], th, [g[0] for g in gr], [g[1] for g in gr])
    assert np.all(st == 0)
    for p in range(2):
        check(7, Q, D, R, pts[p], th[p], gr[p][0], gr[p][1], *out[p])
    ctx.close()


@pytest.mark.parametrize("kidx,Q", [(0, 1), (8, 3)])
def test_single_output_families(kidx, Q):
    pts = [synth.patient(47, p, 1, n) for p, n in enumerate((80, 140))]
    th = np.stack([synth.theta(47, p, kidx, Q, 1, 0) for p in range(2)])
    t2 = [grid(500 + p, 1, pts[p][1], 66)[1] for p in range(2)]
    ctx = make_ctx(kidx, Q, 1, 0, pts)
    out, st = ctx.posterior([0, 1], th, None, t2)
    assert np.all(st == 0)
    for p in range(2):
        mean, var, parts = out[p]
        assert parts.shape == (66, 1)
        np.testing.assert_allclose(parts[:, 0], mean, rtol=1e-5, atol=1e-6 * np.abs(mean).max())
        check(kidx, Q, 1, 0, pts[p], th[p], None, t2[p], mean, var, parts)
    ctx.close()


def test_ragged_point_counts():
    D, Q, R = 3, 2, 2
    pts = [synth.patient(48, p, D, n) for p, n in enumerate((50, 120, 64, 200, 33))]
    th = np.stack([synth.theta(48, p, 7, Q, D, R) for p in range(5)])
    npts = (0, 200, 0, 64, 1)   # empty ranges, four tiles for one patient, exactly one full tile
    gr = [grid(600 + p, D, pts[p][1], k) for p, k in enumerate(npts)]
    ctx = make_ctx(7, Q, D, R, pts)
    out, st = ctx.posterior(np.arange(5), th, [g[0] for g in gr], [g[1] for g in gr])
    assert np.all(st == 0)
    for p in range(5):
        assert out[p][0].shape == (npts[p],) and out[p][2].shape == (npts[p], D)
        check(7, Q, D, R, pts[p], th[p], gr[p][0], gr[p][1], *out[p])
    # no test point at all: statuses only
    out0, st0 = ctx.posterior(np.arange(5), th, [np.zeros(0, np.int32)] * 5, [np.zeros(0, np.float32)] * 5)
    assert np.all(st0 == 0) and all(o[0].shape == (0,) for o in out0)
    ctx.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_point_outputs_are_bit_invariant(monkeypatch):
    D, Q, R = 5, 3, 2
    pts = [synth.patient(49, p, D, n) for p, n in enumerate((150, 300))]
    th = np.stack([synth.theta(49, p, 7, Q, D, R) for p in range(2)])
    gr = [grid(700 + p, D, pts[p][1], k) for p, k in enumerate((100, 150))]
    ctx = make_ctx(7, Q, D, R, pts)
    m2s, t2s = [g[0] for g in gr], [g[1] for g in gr]
    ref, st = ctx.posterior([0, 1], th, m2s, t2s)
    assert np.all(st == 0)
    e0, e1 = np.zeros(0, np.int32), np.zeros(0, np.float32)
    # alone
    for p, j in ((0, 0), (0, 77), (1, 149), (1, 64)):
        one, _ = ctx.posterior([0, 1], th, [m2s[0][j:j + 1] if p == 0 else e0, m2s[1][j:j + 1] if p == 1 else e0],
                               [t2s[0][j:j + 1] if p == 0 else e1, t2s[1][j:j + 1] if p == 1 else e1])
        for k in range(3):
            assert np.array_equal(_bits(one[p][k][0]), _bits(ref[p][k][j])), (p, j, k)
    # shuffled positions
    perm = [np.random.default_rng(1).permutation(len(m2s[p])) for p in range(2)]
    sh, _ = ctx.posterior([0, 1], th, [m2s[p][perm[p]] for p in range(2)], [t2s[p][perm[p]] for p in range(2)])
    for p in range(2):
        for k in range(3):
            assert np.array_equal(_bits(sh[p][k]), _bits(ref[p][k][perm[p]])), (p, k)
    # without the decomposition: the same mean and var bits
    nop, _ = ctx.posterior([0, 1], th, m2s, t2s, parts=False)
    for p in range(2):
        assert nop[p][2] is None
        assert np.array_equal(_bits(nop[p][0]), _bits(ref[p][0])) and np.array_equal(_bits(nop[p][1]), _bits(ref[p][1]))
    ctx.close()
    # a work budget of one tile per launch chunk
    monkeypatch.setenv("MEDGP_POSTERIOR_BUDGET_GB", "1e-6")
    ctx = make_ctx(7, Q, D, R, pts)
    ctx.profile_enable(True, only="k_posterior")
    ch, _ = ctx.posterior([0, 1], th, m2s, t2s)
    launches = ctx.profile_read()["k_posterior"][1]
    assert launches == 2 + 3   # one per tile
    for p in range(2):
        for k in range(3):
            assert np.array_equal(_bits(ch[p][k]), _bits(ref[p][k])), (p, k)
    ctx.close()


def test_failed_entry_gives_nan_and_spares_batch_mates():
    D, Q, R = 2, 2, 2
    sing = (np.zeros(6, np.int32), np.array([1, 1, 1, 2, 2, 2], np.float32), np.ones(6, np.float32))
    good = [synth.patient(50, p, D, n) for p, n in enumerate((40, 90))]
    pts = [good[0], sing, good[1]]
    th = np.stack([synth.theta(50, p, 7, Q, D, R) for p in range(3)])
    th[1, :D] = -80.0   # no noise: the reference's jitter loop gives up (status -1)
    gr = [grid(800 + p, D, pts[p][1], 20) for p in range(3)]
    ctx = make_ctx(7, Q, D, R, pts)
    out, st = ctx.posterior([0, 1, 2], th, [g[0] for g in gr], [g[1] for g in gr])
    assert st[1] < 0 and st[0] == 0 and st[2] == 0
    assert all(np.all(np.isnan(a)) for a in out[1])
    for p in (0, 2):
        check(7, Q, D, R, pts[p], th[p], gr[p][0], gr[p][1], *out[p])
    ctx.close()


def test_capacity_error(monkeypatch):
    monkeypatch.setenv("MEDGP_MEM_BUDGET_GB", "0.0001")   # 107 kB: one 128 x 128 entry pair per wave
    D, Q, R = 2, 2, 2
    pts = [synth.patient(51, p, D, 100) for p in range(3)]
    th = np.stack([synth.theta(51, p, 7, Q, D, R) for p in range(3)])
    gr = [grid(900 + p, D, pts[p][1], 5) for p in range(3)]
    ctx = make_ctx(7, Q, D, R, pts)
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.posterior([0, 1, 2], th, [g[0] for g in gr], [g[1] for g in gr])
    assert "memory budget" in str(e.value) and "-4" in str(e.value)
    ctx.close()
