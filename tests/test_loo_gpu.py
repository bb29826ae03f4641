"""medgp_loo_batch on the MI355X: leave-one-out / leave-group-out predictions against the refit restatement (loo_ref.py) for
every family, kernel variant and grouping scheme of loo_cases.py, the all-inclusive group against medgp_nlml_grad, singleton
bit equality, per-group bit invariance, jitter retries, failed entries beside an asynchronous gradient lane, and one larger
shape."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
from medgp_amd import synth
import loo_cases as LC
import loo_ref as LR


def make_ctx(kidx, Q, D, R, pts):
    ctx = medgp_amd.Context(kidx, Q, D, R)
    ctx.reserve(len(pts), max(max(p[1].shape[0] for p in pts), 1), len(pts))
    for s, (m, t, y) in enumerate(pts):
        ctx.set_patient(s, m if kidx == 7 else None, t, y)
    return ctx


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _report(what, e):
    print(f"LOO-ERR {what}: mean {e[0]:.3g} ulp, var {e[1]:.3g} ulp, lpd {e[2]:.3g} rel")


@pytest.mark.parametrize("i", range(len(LC.CASES)), ids=[LC.case_id(s) for s in LC.CASES])
def test_parity_with_refit(i):
    kidx, Q, D, R, ns, scheme = LC.CASES[i]
    pts, th, gs, ngs = LC.case_data(i)
    ctx = make_ctx(kidx, Q, D, R, pts)
    out, st, gst = ctx.loo(np.arange(len(ns)), th, LC.call_groups(i))
    ctx.close()
    assert np.all(st == 0), st
    worst = (0.0, 0.0, 0.0)
    for p in range(len(ns)):
        assert gst[p].shape == (ngs[p],) and np.all(gst[p] == 0), (p, gst[p])
        assert out[p][0].dtype == np.float32 and out[p][1].dtype == np.float32 and out[p][2].dtype == np.float64
        e = LR.errors(LC.case_ref(i, p), pts[p][2], out[p])
        worst = tuple(max(a, b) for a, b in zip(worst, e))
    _report(LC.case_id(LC.CASES[i]), worst)
    for p in range(len(ns)):
        LR.check_loo(LC.case_ref(i, p), pts[p][2], out[p])
        if gs[p] is not None:   # an empty group: exactly 0.0
            empty = np.bincount(gs[p][gs[p] >= 0], minlength=ngs[p]) == 0
            assert np.all(out[p][2][empty] == 0.0)


ALL = [i for i, s in enumerate(LC.CASES) if s[5] == "all"][0]


def test_all_inclusive_group_is_the_marginal_likelihood():
    """one group of everything: lpd = -nlml of medgp_nlml_grad without a prior (1e-10 relative), var = diag(K), mean = 0.
    medgp_nlml_grad refuses patients of fewer than three observations (the reference's guard): those are held to the refit
    alone (test_parity_with_refit)."""
    kidx, Q, D, R, ns, _ = LC.CASES[ALL]
    pts, th, gs, _ = LC.case_data(ALL)
    ctx = make_ctx(kidx, Q, D, R, pts)
    slots = np.arange(len(ns))
    out, st, gst = ctx.loo(slots, th, gs)
    nlml, _, st_n = ctx.nlml_grad(slots, th, False)
    ctx.close()
    assert np.all(st == 0)
    compared = 0
    for p, n in enumerate(ns):
        K = LR.gram(kidx, Q, D, R, pts[p][0], pts[p][1], th[p])
        dk = np.diag(K)
        assert np.all(np.abs(out[p][1].astype(np.float64) - dk) <= 2.0 ** -22 * np.maximum(dk, 1e-3 * dk.max())), p
        assert np.all(np.abs(out[p][0]) <= 2.0 ** -22 * 1e-3 * np.abs(pts[p][2]).max()), p
        assert out[p][3] == out[p][2][0]
        if st_n[p] >= 0:
            assert abs(out[p][2][0] + nlml[p]) <= 1e-10 * abs(nlml[p]), (p, out[p][2][0], nlml[p])
            compared += 1
    assert compared == sum(1 for n in ns if n >= 3)


def test_explicit_singletons_give_the_bits_of_null():
    kidx, Q, D, R, ns, _ = LC.CASES[0]
    pts, th, _, _ = LC.case_data(0)
    ctx = make_ctx(kidx, Q, D, R, pts)
    slots = np.arange(len(ns))
    a, st, _ = ctx.loo(slots, th, None)
    b, _, _ = ctx.loo(slots, th, [np.arange(n, dtype=np.int32) for n in ns])
    c, _, _ = ctx.loo(slots, th, [np.arange(n, dtype=np.int32)[::-1].copy() for n in ns])
    ctx.close()
    assert np.all(st == 0)
    for p in range(len(ns)):
        for k in range(3):
            assert _same_bits(a[p][k], b[p][k]), (p, k)
        assert _same_bits(a[p][0], c[p][0]) and _same_bits(a[p][1], c[p][1]) and _same_bits(a[p][2], c[p][2][::-1].copy())
        assert a[p][3] == b[p][3]


def _by_group(out_p, ids):
    """{frozenset of members: (mean of the members, var of the members, lpd)} of one patient's output"""
    d = {}
    for gid in np.unique(ids[ids >= 0]):
        B = np.flatnonzero(ids == gid)
        d[frozenset(B.tolist())] = (out_p[0][B], out_p[1][B], out_p[2][gid:gid + 1])
    return d


def _assert_groups_equal(ref_p, ids_ref, out_p, ids, what):
    a, b = _by_group(ref_p, ids_ref), _by_group(out_p, ids)
    common = set(a) & set(b)
    assert common, what
    for key in common:
        for k in range(3):
            assert _same_bits(a[key][k], b[key][k]), (what, sorted(key)[:4], k)
    return len(common)


def test_group_outputs_are_bit_invariant(monkeypatch):
    """relabelled groups, groups added / removed, reordered patients, a patient alone, and launch chunks forced by a tiny
    budget: the same bits per group (route pinned)"""
    fam, pts, th, gs = LC.invariance_case()
    P = len(pts)
    ctx = make_ctx(*fam, pts)
    ctx.pin_route(True)
    ctx.profile_enable(True)
    ref, st, gst = ctx.loo(np.arange(P), th, gs)
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    assert np.all(st == 0) and all(np.all(g == 0) for g in gst)
    classes = len(ctx.last_plan())
    assert prof["k_loo_gram"][1] == classes and prof["k_postfactor"][1] == classes and prof["k_loo_solve"][1] == classes, prof
    assert prof["k_loo_diag"][1] == 0, prof
    # relabelled: id g -> 4 - g
    rel = [4 - g for g in gs]
    out, _, _ = ctx.loo(np.arange(P), th, rel)
    for p in range(P):
        assert _assert_groups_equal(ref[p], gs[p], out[p], rel[p], "relabelled") == 5
    # other groups removed (-1), split into singletons, or merged: groups 0 and 1 keep their members
    for what, f in (("removed", lambda g: np.where(g <= 1, g, -1)),
                    ("split", lambda g: np.where(g <= 1, g, 2 + np.arange(g.shape[0]))),
                    ("merged", lambda g: np.where(g <= 1, g, 2))):
        alt = [f(g).astype(np.int32) for g in gs]
        out, _, _ = ctx.loo(np.arange(P), th, alt)
        for p in range(P):
            assert _assert_groups_equal(ref[p], gs[p], out[p], alt[p], what) >= 2
    # reordered patients, a patient alone
    r = np.arange(P)[::-1]
    out, _, _ = ctx.loo(r, th[r], [gs[p] for p in r])
    for i, p in enumerate(r):
        for k in range(3):
            assert _same_bits(out[i][k], ref[p][k]), ("reversed", p, k)
        assert out[i][3] == ref[p][3]
    for p in range(P):
        out, _, _ = ctx.loo([p], th[p:p + 1], [gs[p]])
        for k in range(3):
            assert _same_bits(out[0][k], ref[p][k]), ("alone", p, k)
    ctx.close()
    # 4e-4 GB = 429 kB: a group of up to 64 observations needs 66.5 kB, one of 65 to 128 264 kB -- the ten groups of the two
    # patients of the largest class (about 60 observations each) no longer share a launch chunk
    monkeypatch.setenv("MEDGP_POSTERIOR_BUDGET_GB", "4e-4")
    ctx = make_ctx(*fam, pts)
    ctx.pin_route(True)
    ctx.profile_enable(True)
    ch, st2, gst2 = ctx.loo(np.arange(P), th, gs)
    prof = ctx.profile_read()
    ctx.close()
    assert np.all(st2 == 0) and all(np.all(g == 0) for g in gst2)
    assert prof["k_loo_gram"][1] > classes and prof["k_loo_gram"][1] == prof["k_postfactor"][1] == prof["k_loo_solve"][1], prof
    for p in range(P):
        for k in range(3):
            assert _same_bits(ch[p][k], ref[p][k]), ("chunked", p, k)
        assert ch[p][3] == ref[p][3]
    for p in range(P):
        LR.check_loo(LR.refit(*LC.family_args(fam, pts[p]), th[p], gs[p], 5), pts[p][2], ref[p])


def test_single_group_beyond_the_budget_is_a_capacity_error(monkeypatch):
    monkeypatch.setenv("MEDGP_POSTERIOR_BUDGET_GB", "1e-5")
    fam, pts, th, gs = LC.invariance_case()
    ctx = make_ctx(*fam, pts)
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.loo(np.arange(len(pts)), th, gs)
    assert "MEDGP_POSTERIOR_BUDGET_GB" in str(e.value) and "-4" in str(e.value)   # MEDGP_ERR_CAPACITY
    out, st, _ = ctx.loo(np.arange(len(pts)), th, None)   # singletons need no block
    ctx.close()
    assert np.all(st == 0)


@pytest.mark.parametrize("fails", [1, 3])
def test_jitter_retries(fails, monkeypatch):
    """every quantity is that of the matrix that was factored, K + k diag(sigma^2)"""
    monkeypatch.setenv("MEDGP_DEBUG_FAIL_ATTEMPTS", str(fails))
    fam, pts, th, gs = LC.jitter_case()
    ctx = make_ctx(*fam, pts)
    slots = np.arange(len(pts))
    out, st, gst = ctx.loo(slots, th, gs)
    single, st1, _ = ctx.loo(slots, th, None)
    ctx.close()
    assert np.all(st == fails) and np.all(st1 == fails) and all(np.all(g == 0) for g in gst), (st, gst)
    worst = (0.0, 0.0, 0.0)
    for p in range(len(pts)):
        args = LC.family_args(fam, pts[p])
        ng = int(gs[p].max()) + 1
        worst = tuple(max(a, b) for a, b in zip(worst, LR.check_loo(LR.refit(*args, th[p], gs[p], ng, jitter_rounds=fails), pts[p][2], out[p])))
        worst = tuple(max(a, b) for a, b in zip(worst, LR.check_loo(LR.refit(*args, th[p], jitter_rounds=fails), pts[p][2], single[p])))
    _report(f"jitter{fails}", worst)


def test_exhausted_retries_give_nan(monkeypatch):
    monkeypatch.setenv("MEDGP_DEBUG_FAIL_ATTEMPTS", "11")
    fam, pts, th, gs = LC.jitter_case()
    ctx = make_ctx(*fam, pts)
    for groups in (gs, None):
        out, st, gst = ctx.loo(np.arange(len(pts)), th, groups)
        assert np.all(st == -1) and all(np.all(g == -1) for g in gst)
        for o in out:
            assert all(np.all(np.isnan(a)) for a in o[:3]) and np.isnan(o[3])
    ctx.close()


def test_failed_entry_beside_good_ones_and_a_gradient_lane():
    """a patient without noise fails (status -1, NaN, group_status -1) and spares its batch-mates; a gradient lane in flight
    is not disturbed; medgp_get_factor works after the call (it formed alpha and L^-1).  The failed patient is deliberately one
    that fails on its own (duplicated times, no noise: every retry meets a zero pivot) and not one that fails under
    MEDGP_DEBUG_FAIL_ATTEMPTS: that hook is read once per context and applies to every entry, so it cannot fail one patient
    beside good ones; the status, NaN and group_status paths are the same."""
    fam, pts, th, gs = LC.jitter_case()
    D = fam[2]
    sing = (np.zeros(6, np.int32), np.array([1, 1, 1, 2, 2, 2], np.float32), np.ones(6, np.float32))
    pts = [pts[0], sing, pts[1], pts[3]]
    th = np.stack([th[0], th[2], th[1], th[3]])
    th[1, :D] = -80.0   # no noise: the reference's jitter loop gives up (status -1)
    gs = [gs[0], np.array([0, 0, 1, 1, 2, -1], np.int32), gs[1], gs[3]]
    ctx = make_ctx(*fam, pts)
    good = [0, 2, 3]
    nl_ref, gr_ref, st_ref = ctx.nlml_grad(good, th[good], True)
    H = th.shape[1]
    lane_th = ctx.pinned((3, H), np.float64); lane_th[:] = th[good]
    lane_nl = ctx.pinned((3,), np.float64)
    lane_gr = ctx.pinned((3, H), np.float64)
    lane_st = ctx.pinned((3,), np.int32)
    ctx.nlml_grad_async(0, np.array(good), lane_th, True, lane_nl, lane_gr, lane_st)
    out, st, gst = ctx.loo([0, 1, 2, 3], th, gs)
    ctx.wait(0)
    assert np.array_equal(lane_st, st_ref) and np.array_equal(lane_nl, nl_ref) and np.array_equal(lane_gr, gr_ref)
    assert st[1] < 0 and all(st[p] == 0 for p in good), st
    assert np.all(gst[1] == -1) and all(np.all(gst[p] == 0) for p in good)
    assert all(np.all(np.isnan(a)) for a in out[1][:3]) and np.isnan(out[1][3])
    for p in good:
        LR.check_loo(LR.refit(*LC.family_args(fam, pts[p]), th[p], gs[p], int(gs[p].max()) + 1), pts[p][2], out[p])
    # the factor of the call: alpha and L^-1 in the caller's order (patient 3 is interleaved: re-factored on request)
    for b in good:
        n = pts[b][1].shape[0]
        alpha, linv, _ = ctx.get_factor(b, n)
        K = LR.gram(*LC.family_args(fam, pts[b])[:6], th[b])
        a_ref = np.linalg.solve(K, pts[b][2].astype(np.float64))
        Li_ref = np.linalg.inv(np.linalg.cholesky(K))
        assert np.all(np.abs(alpha - a_ref) <= 1e-5 * np.abs(a_ref).max()), b
        assert np.all(np.abs(linv - Li_ref) <= 1e-5 * np.abs(Li_ref).max()), b
    with pytest.raises(medgp_amd.MedgpError):
        ctx.get_factor(1, 6)   # the failed entry has no factor
    ctx.close()


def test_larger_shape_by_covariate_and_singletons():
    """D = 24, Q = 5, n = 512: the second pass sizes of the factorisation"""
    kidx, Q, D, R, n = 7, 5, 24, 8, 512
    pt = synth.patient(7500, 0, D, n, interleave=True)
    th = synth.theta(7500, 0, kidx, Q, D, R)
    ctx = make_ctx(kidx, Q, D, R, [pt])
    cov, st, gst = ctx.loo([0], th[None, :], "covariate")
    one, st1, _ = ctx.loo([0], th[None, :], None)
    ctx.close()
    assert st[0] == 0 and st1[0] == 0 and np.all(gst[0] == 0)
    args = LC.family_args((kidx, Q, D, R), pt)
    assert LR.cond(LR.gram(*args[:6], th)) <= 1e4
    e1 = LR.check_loo(LR.refit(*args, th, pt[0], D), pt[2], cov[0])
    e2 = LR.check_loo(LR.refit(*args, th), pt[2], one[0])
    _report("n512", tuple(max(a, b) for a, b in zip(e1, e2)))
