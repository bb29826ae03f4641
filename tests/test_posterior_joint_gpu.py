"""medgp_posterior_joint_batch on the MI355X: covariance and sample paths against the fp64 restatement
(posterior_joint_ref.py) for every family and kernel variant, ragged point counts, bit equality of mean / var with
medgp_posterior_batch, per-patient bit invariance, jitter retries, duplicated points, failed entries, launch counts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
import posterior_joint_cases as PC
from posterior_joint_ref import check_joint, restate_joint
from posterior_ref import check_posterior, restate


def make_ctx(kidx, Q, D, R, pts):
    ctx = medgp_amd.Context(kidx, Q, D, R)
    ctx.reserve(len(pts), max(max(p[1].shape[0] for p in pts), 1), len(pts))
    for s, (m, t, y) in enumerate(pts):
        ctx.set_patient(s, m if kidx == 7 else None, t, y)
    return ctx


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _lists(tp, multi=True):
    return ([x[0] for x in tp] if multi else None), [x[1] for x in tp]


def _check_patient(fam, pt, th, tp, out, eps, jitter_rounds=0):
    kidx, Q, D, R = fam
    multi = kidx == 7
    mean, var, cov, samples = out
    args = (kidx, Q, D, R, pt[0] if multi else None, pt[1], pt[2], th, tp[0] if multi else None, tp[1])
    check_posterior(kidx, D, th, tp[0] if multi else None, restate(*args, jitter_rounds=jitter_rounds)[:2] + (None,), mean, var)
    check_joint(restate_joint(*args, jitter_rounds=jitter_rounds), var, cov, samples, eps)


@pytest.mark.parametrize("i", range(len(PC.SHAPES)), ids=[PC.shape_id(s) for s in PC.SHAPES])
def test_parity_with_restatement(i):
    kidx, Q, D, R, ns, ms, nsamp, cov = PC.SHAPES[i]
    pts, th, tp, eps = PC.shape_data(i)
    multi = kidx == 7
    m2s, t2s = _lists(tp, multi)
    ctx = make_ctx(kidx, Q, D, R, pts)
    slots = np.arange(len(ns))
    out, st, cst = ctx.posterior_joint(slots, th, m2s, t2s, eps, cov=cov)
    marg, st_m = ctx.posterior(slots, th, m2s, t2s, parts=False)
    ctx.close()
    assert np.all(st == 0) and np.all(cst == 0) and np.array_equal(st, st_m), (st, cst)
    for p in range(len(ns)):
        mean, var, cv, sm = out[p]
        assert mean.shape == (ms[p],) and var.shape == (ms[p],)
        assert (cv is not None) == cov and (sm is not None) == (nsamp > 0)
        if cov:
            assert cv.shape == (ms[p], ms[p])
        if nsamp:
            assert sm.shape == (ms[p], nsamp)
        # mean and var are medgp_posterior_batch's, bit for bit
        assert _same_bits(mean, marg[p][0]) and _same_bits(var, marg[p][1]), p
        _check_patient((kidx, Q, D, R), pts[p], th[p], tp[p], out[p], eps[p] if nsamp else None)


def test_cov_and_samples_do_not_depend_on_what_else_is_asked():
    fam, pts, th, tp, eps = PC.invariance_case()
    m2s, t2s = _lists(tp)
    ctx = make_ctx(*fam, pts)
    slots = np.arange(len(pts))
    both, _, _ = ctx.posterior_joint(slots, th, m2s, t2s, eps, cov=True)
    conly, _, cst_c = ctx.posterior_joint(slots, th, m2s, t2s, None, cov=True)
    sonly, _, cst_s = ctx.posterior_joint(slots, th, m2s, t2s, eps, cov=False)
    one, _, _ = ctx.posterior_joint(slots, th, m2s, t2s, [e[:, :1] for e in eps], cov=False)
    ctx.close()
    assert np.all(cst_c == 0) and np.all(cst_s == 0)
    for p in range(len(pts)):
        assert _same_bits(conly[p][2], both[p][2]) and conly[p][3] is None
        assert _same_bits(sonly[p][3], both[p][3]) and sonly[p][2] is None
        assert _same_bits(one[p][3], both[p][3][:, :1])      # a path does not depend on the other paths of the call
        for k in (0, 1):
            assert _same_bits(conly[p][k], both[p][k]) and _same_bits(sonly[p][k], both[p][k])


def test_patient_outputs_are_bit_invariant(monkeypatch):
    """reversed patients, a patient alone, and launch chunks of one patient each: the same bits per patient"""
    fam, pts, th, tp, eps = PC.invariance_case()
    m2s, t2s = _lists(tp)
    P = len(pts)
    ctx = make_ctx(*fam, pts)
    ctx.profile_enable(True)
    ref, st, cst = ctx.posterior_joint(np.arange(P), th, m2s, t2s, eps)
    ref_launches = ctx.profile_read()["k_postcov"][1]
    ctx.profile_enable(False)
    assert np.all(st == 0) and np.all(cst == 0)
    assert ref_launches == len(ctx.last_plan()) == 3     # one chunk per size class
    r = np.arange(P)[::-1]
    rev, _, _ = ctx.posterior_joint(r, th[r], [m2s[p] for p in r], [t2s[p] for p in r], [eps[p] for p in r])
    for i, p in enumerate(r):
        for k in range(4):
            assert _same_bits(rev[i][k], ref[p][k]), ("reversed", p, k)
    for p in range(P):
        alone, _, _ = ctx.posterior_joint([p], th[p:p + 1], [m2s[p]], [t2s[p]], [eps[p]])
        for k in range(4):
            assert _same_bits(alone[0][k], ref[p][k]), ("alone", p, k)
    ctx.close()
    # 1e-3 GB: the two patients of the largest class (0.85 and 0.7 MB of work rows, C and cov) no longer share a chunk
    monkeypatch.setenv("MEDGP_POSTERIOR_BUDGET_GB", "1e-3")
    ctx = make_ctx(*fam, pts)
    ctx.profile_enable(True)
    ch, st2, cst2 = ctx.posterior_joint(np.arange(P), th, m2s, t2s, eps)
    prof = ctx.profile_read()
    ctx.close()
    assert np.all(st2 == 0) and np.all(cst2 == 0)
    assert prof["k_postcov"][1] == 4 and prof["k_posterior"][1] == 4 and prof["k_postfactor"][1] == 4 and prof["k_postdraw"][1] == 4, prof
    for p in range(P):
        for k in range(4):
            assert _same_bits(ch[p][k], ref[p][k]), ("chunked", p, k)
    for p in range(P):
        _check_patient(fam, pts[p], th[p], tp[p], ref[p], eps[p])


def test_single_patient_beyond_the_budget_is_a_capacity_error(monkeypatch):
    monkeypatch.setenv("MEDGP_POSTERIOR_BUDGET_GB", "1e-4")
    fam, pts, th, tp, eps = PC.invariance_case()
    m2s, t2s = _lists(tp)
    ctx = make_ctx(*fam, pts)
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.posterior_joint(np.arange(len(pts)), th, m2s, t2s, eps)
    assert "MEDGP_POSTERIOR_BUDGET_GB" in str(e.value) and "-4" in str(e.value)
    # the marginals of the same points still run (tile by tile)
    out, st = ctx.posterior(np.arange(len(pts)), th, m2s, t2s)
    assert np.all(st == 0)
    ctx.close()


@pytest.mark.parametrize("fails", [1, 3])
def test_jitter_retries(fails, monkeypatch):
    """C is that of the factor of K + k diag(sigma^2); the test points' noise is still added once"""
    monkeypatch.setenv("MEDGP_DEBUG_FAIL_ATTEMPTS", str(fails))
    fam, pts, th, tp, eps = PC.jitter_case()
    m2s, t2s = _lists(tp)
    ctx = make_ctx(*fam, pts)
    out, st, cst = ctx.posterior_joint(np.arange(len(pts)), th, m2s, t2s, eps)
    ctx.close()
    assert np.all(st == fails) and np.all(cst == 0), (st, cst)
    for p in range(len(pts)):
        _check_patient(fam, pts[p], th[p], tp[p], out[p], eps[p], jitter_rounds=fails)


def test_exhausted_retries_give_nan(monkeypatch):
    monkeypatch.setenv("MEDGP_DEBUG_FAIL_ATTEMPTS", "11")
    fam, pts, th, tp, eps = PC.jitter_case()
    m2s, t2s = _lists(tp)
    ctx = make_ctx(*fam, pts)
    out, st, cst = ctx.posterior_joint(np.arange(len(pts)), th, m2s, t2s, eps)
    ctx.close()
    assert np.all(st == -1) and np.all(cst == -1)
    for o in out:
        assert all(np.all(np.isnan(a)) for a in o)


def test_duplicated_points_and_points_on_training_points():
    fam, pt, th, tp, eps = PC.duplicates_case()
    ctx = make_ctx(*fam, [pt])
    out, st, cst = ctx.posterior_joint([0], th[None, :], [tp[0]], [tp[1]], [eps])
    ctx.close()
    assert st[0] == 0 and cst[0] == 0
    _check_patient(fam, pt, th, tp, out[0], eps)
    cov = out[0][2]
    # duplicated test points: the same rows of cov but for the noise on their own diagonal entries
    a, b = np.arange(40, 50), np.arange(100, 110)
    others = np.setdiff1d(np.arange(cov.shape[0]), np.concatenate([a, b]))
    assert np.array_equal(_bits(cov[np.ix_(a, others)]), _bits(cov[np.ix_(b, others)]))


def test_interleaved_with_an_asynchronous_gradient_lane():
    fam, pts, th, tp, eps = PC.jitter_case()
    m2s, t2s = _lists(tp)
    ctx = make_ctx(*fam, pts)
    args = (np.arange(len(pts)), th, m2s, t2s, eps)
    ref, st, cst = ctx.posterior_joint(*args)
    assert np.all(st == 0) and np.all(cst == 0)
    sel = [3, 1, 0]
    nl_ref, gr_ref, st_ref = ctx.nlml_grad(sel, th[sel], True)
    H = th.shape[1]
    lane_th = ctx.pinned((3, H), np.float64); lane_th[:] = th[sel]
    lane_nl = ctx.pinned((3,), np.float64)
    lane_gr = ctx.pinned((3, H), np.float64)
    lane_st = ctx.pinned((3,), np.int32)
    ctx.nlml_grad_async(0, np.array(sel), lane_th, True, lane_nl, lane_gr, lane_st)
    mid, st_mid, cst_mid = ctx.posterior_joint(*args)
    ctx.wait(0)
    assert np.array_equal(st_mid, st) and np.array_equal(cst_mid, cst) and np.array_equal(lane_st, st_ref)
    assert np.array_equal(lane_nl, nl_ref) and np.array_equal(lane_gr, gr_ref)
    # joint -> posterior -> nlml_grad(keep_factor) -> joint
    ctx.posterior(*args[:4])
    ctx.nlml_grad(np.arange(len(pts))[::-1], th[::-1], False, keep_factor=True)
    after, _, _ = ctx.posterior_joint(*args)
    ctx.close()
    for p in range(len(pts)):
        for k in range(4):
            assert _same_bits(mid[p][k], ref[p][k]) and _same_bits(after[p][k], ref[p][k]), (p, k)
    for p in range(len(pts)):
        _check_patient(fam, pts[p], th[p], tp[p], ref[p], eps[p])


def test_failed_entry_gives_nan_and_spares_batch_mates():
    fam, pts, th, tp, eps = PC.jitter_case()
    D = fam[2]
    sing = (np.zeros(6, np.int32), np.array([1, 1, 1, 2, 2, 2], np.float32), np.ones(6, np.float32))
    pts = [pts[0], sing, pts[1]]
    th = np.stack([th[0], th[2], th[1]])
    th[1, :D] = -80.0   # no noise: the reference's jitter loop gives up (status -1)
    tp = [tp[0], tp[3], tp[1]]
    eps = [eps[0], eps[3], eps[1]]
    m2s, t2s = _lists(tp)
    ctx = make_ctx(*fam, pts)
    for kw in ({"eps_list": eps, "cov": True}, {"eps_list": None, "cov": True}, {"eps_list": eps, "cov": False}):
        out, st, cst = ctx.posterior_joint([0, 1, 2], th, m2s, t2s, **kw)
        assert st[1] < 0 and st[0] == 0 and st[2] == 0 and list(cst) == [0, -1, 0], (st, cst)
        assert all(np.all(np.isnan(a)) for a in out[1] if a is not None)
        for p in (0, 2):
            _check_patient(fam, pts[p], th[p], tp[p], out[p], eps[p] if kw["eps_list"] is not None else None)
    ctx.close()


def test_launch_counts():
    """k_postcov whenever cov or samples are asked for; the factorisation of C and k_postdraw only with samples"""
    fam, pts, th, tp, eps = PC.jitter_case()
    m2s, t2s = _lists(tp)
    ctx = make_ctx(*fam, pts)
    ctx.profile_enable(True)
    args = (np.arange(len(pts)), th, m2s, t2s)
    ctx.posterior_joint(*args, None, cov=True)
    classes = len(ctx.last_plan())
    prof = ctx.profile_read()
    assert prof["k_postcov"][1] == classes and prof["k_postfactor"][1] == 0 and prof["k_postdraw"][1] == 0, prof
    ctx.profile_reset()
    ctx.posterior_joint(*args, eps, cov=False)
    prof = ctx.profile_read()
    assert prof["k_postcov"][1] == classes and prof["k_postfactor"][1] == classes and prof["k_postdraw"][1] == classes, prof
    ctx.profile_reset()
    ctx.posterior(*args)
    prof = ctx.profile_read()
    assert prof["k_posterior"][1] == classes and prof["k_postcov"][1] == 0 and prof["k_postfactor"][1] == 0 and prof["k_postdraw"][1] == 0, prof
    # no test point at all: statuses only, nothing joint launched
    ctx.profile_reset()
    e0 = [np.zeros(0, np.int32)] * len(pts), [np.zeros(0, np.float32)] * len(pts)
    out, st, cst = ctx.posterior_joint(np.arange(len(pts)), th, *e0, [np.zeros((0, 3))] * len(pts))
    prof = ctx.profile_read()
    assert np.all(st == 0) and np.all(cst == 0) and all(o[2].shape == (0, 0) and o[3].shape == (0, 3) for o in out)
    assert prof["k_postcov"][1] == 0 and prof["k_postdraw"][1] == 0, prof
    ctx.close()
