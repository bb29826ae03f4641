"""medgp_mean_nlml_grad / medgp_mean_posterior_batch on the MI355X against the long-double truth (mean_truth.py) within the fp64 budget
measured on CPU programs alone: every case of mean_truth (n = 3, 63, 64, 65, 130; D = 1 through SM and SE, 3, 24, 33, 64; Q = 5 and 9;
lam mixed per covariate including 0; covariates without observations; covariates interleaved) as one ragged batch in both modes on
the default, the pinned and the look-ahead route; an improper entry and a failed factorisation beside healthy batch-mates; one and
three jitter rounds; a theta prior; FIXED at zero against medgp_nlml_grad; bit invariance with the route pinned; argument and
capacity errors; and the older calls' bits right behind the new call."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
import mean_truth as MT
import nlml_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ["auto", "pinned", "la"]
MODES = [MT.MARGINAL, MT.FIXED]
MODE_NAME = {MT.MARGINAL: "marginal", MT.FIXED: "fixed"}
X = np.longdouble


def make_ctx(fam, pts, route="auto", max_batch=None):
    kidx = fam[0]
    ctx = medgp_amd.Context(*fam)
    ctx.reserve(len(pts), max(max(p[1].shape[0] for p in pts), 1), max_batch or len(pts))
    for s, (m, t, y) in enumerate(pts):
        ctx.set_patient(s, m if kidx == 7 else None, t, y)
    if route == "pinned":
        ctx.pin_route(True)
    return ctx


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in ("nlml", "grad", "dmean", "beta", "beta_cov") if a[k] is not None)


def _kw(c, ps, mode):
    """the baseline arguments of patients ps of a case"""
    b0 = np.stack([c["b0"][p] for p in ps])
    return dict(b0=b0, fixed=True) if mode == MT.FIXED else dict(b0=b0, lam=np.stack([c["lam"][p] for p in ps]))


def _points(c, ps):
    pp = [MT.points(c, p) for p in ps]
    return ([x[0] for x in pp] if c["kidx"] == 7 else None), [x[1] for x in pp]


def _row(r, i):
    return {k: (None if r[k] is None else r[k][i]) for k in ("nlml", "grad", "dmean", "beta", "beta_cov")}


def _hold(c, p, mode, got, what, jitter_rounds=0, post=None):
    """one patient's device outputs against the truth within the budgets; prints error / budget per output"""
    tr, bud = MT.budget_of(c, p, mode, jitter_rounds)
    e = MT.errors(got, tr)
    if post is not None:
        e.update(MT.post_errors(post[0], post[1], tr["post"]))
    assert np.any(tr["grad"] != 0) and np.isfinite(float(tr["nlml"]))     # nothing passes against zeros
    rows = []
    for k, v in e.items():
        print(f"MEAN-ERR {what} {MODE_NAME[mode]} {c['id']}:{p} n {c['pts'][p][1].shape[0]} {k}: {v:.3g} / {bud[k]:.3g}")
        rows.append((what, c["id"], p, k, v, bud[k]))
    return rows


def _assert_held(rows):
    bad = [r for r in rows if not r[4] <= r[5]]
    assert not bad, bad


_LEGS = [(s[0], r) for s in MT._SPECS for r in ROUTES if r != "la" or max(n for n, _ in s[5]) > 128]


@pytest.mark.parametrize("mode", MODES, ids=[MODE_NAME[m] for m in MODES])
@pytest.mark.parametrize("cid,route", _LEGS, ids=[f"{c}-{r}" for c, r in _LEGS])
def test_device_within_budget(cid, route, mode, monkeypatch):
    """every case as one ragged batch in a shuffled order: nlml, grad, dmean, beta, beta_cov and the posterior within budget; the
    posterior also against Context.posterior plus the baseline's share; flag_grad = 0 gives the same bits of what it returns"""
    c = MT.case(cid)
    fam = MT.fam(c)
    P = len(c["pts"])
    if route == "la":
        monkeypatch.setenv("MEDGP_MULTI_CU", "1")
    order = np.roll(np.arange(P), 2)[::-1].copy()
    th = np.stack(c["th"])
    kw = _kw(c, order, mode)
    m2l, t2l = _points(c, order)
    ctx = make_ctx(fam, c["pts"], route)
    r = ctx.mean_nlml_grad(order, th[order], **kw)
    r0 = ctx.mean_nlml_grad(order, th[order], flag_grad=False, **kw)
    post, pbeta, pst = ctx.mean_posterior(order, th[order], m2l, t2l, **kw)
    plain, plain_st = ctx.posterior(order, th[order], m2l, t2l, parts=False)
    ctx.close()
    rows = []
    for i, p in enumerate(order):
        tr = MT.truth_of(c, p, mode)
        n = c["pts"][p][1].shape[0]
        assert r["status"][i] == tr["status"] == 0 and pst[i] == 0 and r0["status"][i] == 0, (p, r["status"], pst)
        assert r0["grad"] is None and all(np.array_equal(_bits(r0[k][i]), _bits(r[k][i])) for k in ("nlml", "dmean", "beta", "beta_cov"))
        assert np.array_equal(_bits(pbeta[i]), _bits(r["beta"][i]))
        rows += _hold(c, p, mode, _row(r, i), route, post=post[i])
        # against the zero-mean posterior call (float outputs, its own bar of 2 fp32 ulps) plus the truth's shares of the baseline
        tp = tr["post"]
        s_m, s_v = float(np.abs(tp["mean0"]).max()), float(np.abs(tp["var0"]).max())
        assert np.all(np.abs(post[i][0] - (plain[i][0].astype(np.float64) + tp["dmean"].astype(np.float64))) <= 4 * 2.0 ** -23 * np.maximum(np.abs(tp["mean0"]).astype(np.float64), 1e-3 * s_m) + 1e-9), (p, n)
        assert np.all(np.abs(post[i][1] - (plain[i][1].astype(np.float64) + tp["extra"].astype(np.float64))) <= 4 * 2.0 ** -23 * np.maximum(np.abs(tp["var0"]).astype(np.float64), 1e-3 * s_v) + 1e-9), (p, n)
        if mode == MT.FIXED:
            assert np.array_equal(_bits(r["beta"][i]), _bits(c["b0"][p])) and not r["beta_cov"][i].any()
    _assert_held(rows)


def test_improper_entry_and_failed_factorisation_spare_their_batch_mates():
    """lmc_D24:0 has covariates without observations: lam = 0 on one of them is improper (status -1, NaN, decided on the device), and
    lam > 0 there is healthy; a non-finite theta fails the factorisation of another entry.  With the route pinned the healthy
    batch-mates keep their bits in both calls."""
    c = MT.case("lmc_D24")
    fam = MT.fam(c)
    m = c["pts"][0][0]
    absent = int(np.where(np.bincount(m, minlength=c["D"]) == 0)[0][0])
    ps = [0, 1, 0, 1]
    th = np.stack([c["th"][p] for p in ps])
    kw = _kw(c, ps, MT.MARGINAL)
    assert kw["lam"][0, absent] > 0
    m2l, t2l = _points(c, ps)
    m2l[0] = np.concatenate([m2l[0], [absent]]).astype(np.int32)        # a point on the unobserved covariate
    t2l[0] = np.concatenate([t2l[0], [50.0]]).astype(np.float32)
    ctx = make_ctx(fam, [c["pts"][p] for p in ps], "pinned")
    sl = np.arange(4)
    good = ctx.mean_nlml_grad(sl, th, **kw)
    gpost, _, gst = ctx.mean_posterior(sl, th, m2l, t2l, **kw)
    assert np.all(good["status"] == 0) and np.all(gst == 0)
    # lam > 0 on the unobserved covariate: beta^ = b0 there, A^-1 has 1 / lam on its diagonal and nothing beside it
    assert good["beta"][0, absent] == kw["b0"][0, absent] and good["dmean"][0, absent] == 0
    assert abs(good["beta_cov"][0, absent, absent] * kw["lam"][0, absent] - 1) <= 1e-15
    assert not np.delete(good["beta_cov"][0, absent], absent).any()
    tp = MT.posterior(*fam, *c["pts"][0], c["th"][0], MT.MARGINAL, kw["b0"][0], kw["lam"][0], m2l[0], t2l[0], X)
    assert tp["extra"][-1] >= 1 / X(kw["lam"][0, absent])
    assert abs(gpost[0][1][-1] - float(tp["var"][-1])) <= 2.0 ** -30 * float(tp["mag_var"][-1])
    bad = dict(kw, lam=kw["lam"].copy())
    bad["lam"][2, absent] = 0.0                                          # entry 2 improper
    thf = th.copy()
    thf[3, 0] = np.nan                                                   # entry 3 does not factor
    r = ctx.mean_nlml_grad(sl, thf, **bad)
    post, pbeta, pst = ctx.mean_posterior(sl, thf, m2l, t2l, **bad)
    rf = ctx.mean_nlml_grad(sl, thf, b0=kw["b0"], fixed=True)           # FIXED ignores lam: entry 2 is healthy there
    ctx.close()
    assert list(r["status"]) == [0, 0, -1, -1] and list(pst) == [0, 0, -1, -1] and list(rf["status"]) == [0, 0, 0, -1]
    for i in (2, 3):
        assert all(np.all(np.isnan(r[k][i])) for k in ("nlml", "grad", "dmean", "beta", "beta_cov")), i
        assert np.all(np.isnan(post[i][0])) and np.all(np.isnan(post[i][1])) and np.all(np.isnan(pbeta[i]))
    for i in (0, 1):
        assert _same(_row(r, i), _row(good, i)), i
        assert np.array_equal(_bits(post[i][0]), _bits(gpost[i][0])) and np.array_equal(_bits(post[i][1]), _bits(gpost[i][1]))
    assert np.all(np.isfinite(rf["grad"][2])) and np.all(np.isnan(rf["grad"][3]))


def test_bit_invariance_with_the_route_pinned():
    """an entry's bits depend on its own operands alone: alone, in a batch of 7, reversed, at another position; a point's not on the
    other points or their order"""
    c = MT.case("lmc_D3_Q5")
    fam = MT.fam(c)
    ctx = make_ctx(fam, c["pts"], "pinned", max_batch=7)
    for mode in MODES:
        batch = [4, 1, 2, 4, 3, 0, 1]
        th = np.stack([c["th"][p] for p in batch])
        m2l, t2l = _points(c, batch)
        full = ctx.mean_nlml_grad(batch, th, **_kw(c, batch, mode))
        fpost, _, _ = ctx.mean_posterior(batch, th, m2l, t2l, **_kw(c, batch, mode))
        rev = ctx.mean_nlml_grad(batch[::-1], th[::-1], **_kw(c, batch[::-1], mode))
        assert _same(_row(full, 0), _row(full, 3)) and _same(_row(full, 1), _row(full, 6))   # another position
        for i, p in enumerate(batch):
            assert _same(_row(rev, 6 - i), _row(full, i)), (mode, i)
            one = ctx.mean_nlml_grad([p], th[i:i + 1], **_kw(c, [p], mode))
            assert _same(_row(one, 0), _row(full, i)), (mode, i)
        # the points of patient 4 reversed and alone
        pr, _, _ = ctx.mean_posterior([4], th[:1], None if m2l is None else [m2l[0][::-1].copy()], [t2l[0][::-1].copy()], **_kw(c, [4], mode))
        assert np.array_equal(_bits(pr[0][0][::-1]), _bits(fpost[0][0])) and np.array_equal(_bits(pr[0][1][::-1]), _bits(fpost[0][1]))
    ctx.close()


def test_fixed_at_zero_is_the_plain_nlml_within_the_two_budgets():
    """FIXED with b0 = 0 is medgp_nlml_grad's model: both calls meet the same truth, each within its own budget (other summation
    orders: not bits)"""
    rows = []
    for cid in ("lmc_D3_Q5", "sm_Q3", "se"):
        c = MT.case(cid)
        fam = MT.fam(c)
        P = len(c["pts"])
        th = np.stack(c["th"])
        ctx = make_ctx(fam, c["pts"])
        r = ctx.mean_nlml_grad(np.arange(P), th, b0=np.zeros(MT.nout(c["kidx"], c["D"])), fixed=True)
        nl, g, st = ctx.nlml_grad(np.arange(P), th, True)
        ctx.close()
        for p in range(P):
            m, t, y = c["pts"][p]
            _, tn, tg = T.nlml_grad(*fam, m, t, y, th[p], X)
            pr = MT.programs_for(c, p, MT.FIXED, np.zeros(MT.nout(c["kidx"], c["D"])), None)
            assert abs(pr["truth"]["nlml"] - tn) <= 1e-17 * abs(tn)
            bud = MT.budgets(pr)
            e1 = MT.errors(_row(r, p), pr["truth"])
            # medgp_nlml_grad's own budget from nlml_truth's float64 programs (b) and (c)
            eb = [T.error_pair(*T.float64_program(c, p, 0, v)[1:], tn, tg) for v in ("plain", "device")]
            bn, bg = min(T.budget([x[0] for x in eb], T.M_NLML), T.NLML_BUDGET_CAP), min(T.budget([x[1] for x in eb], T.M_GRAD), T.GRAD_BUDGET_CAP)
            e2 = T.error_pair(nl[p], g[p], tn, tg)
            assert st[p] == 0 and r["status"][p] == 0
            print(f"MEAN-ERR fixed0 {cid}:{p} mean call nlml {e1['nlml']:.3g} / {bud['nlml']:.3g} grad {e1['grad']:.3g} / {bud['grad']:.3g}; nlml_grad nlml {e2[0]:.3g} / {bn:.3g} grad {e2[1]:.3g} / {bg:.3g}")
            rows += [("fixed0", cid, p, "nlml", e1["nlml"], bud["nlml"]), ("fixed0", cid, p, "grad", e1["grad"], bud["grad"]),
                     ("nlml_grad", cid, p, "nlml", e2[0], bn), ("nlml_grad", cid, p, "grad", e2[1], bg)]
            assert np.any(r["dmean"][p] != 0)     # (an unobserved covariate has a zero line)
    _assert_held(rows)


_CHILD = r"""
import sys
import numpy as np
import medgp_amd
sys.path.insert(0, sys.argv[3])
import mean_truth as MT
from test_mean_gpu import make_ctx, _kw, _points
c = MT.case("lmc_D3_Q5")
ps = [1, 2, 3, 4]
th = np.stack([c["th"][p] for p in ps])
ctx = make_ctx(MT.fam(c), [c["pts"][p] for p in ps], "pinned")
res = {}
for mode in (0, 1):
    r = ctx.mean_nlml_grad(np.arange(4), th, **_kw(c, ps, mode))
    m2l, t2l = _points(c, ps)
    post, _, pst = ctx.mean_posterior(np.arange(4), th, m2l, t2l, **_kw(c, ps, mode))
    res.update({f"{k}{mode}": r[k] for k in r})
    res[f"pst{mode}"] = pst
    for i in range(4):
        res[f"pm{mode}_{i}"], res[f"pv{mode}_{i}"] = post[i]
ctx.close()
np.savez(sys.argv[2], **res)
"""
_CHILD_PS = [1, 2, 3, 4]


@pytest.mark.parametrize("rounds", [1, 3])
def test_jitter_rounds(rounds, tmp_path):
    """every quantity is that of the matrix that was factored, K + k diag(sigma^2), the derivatives un-jittered and the noise lines
    not scaled; the hook is read when the library creates a context, in a process of its own"""
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), MEDGP_DEBUG_FAIL_ATTEMPTS=str(rounds))
    out = str(tmp_path / "jit.npz")
    pr = subprocess.run([sys.executable, "-c", _CHILD, "jitter", out, os.path.join(ROOT, "tests")], env=e, capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr[-2000:]
    z = np.load(out)
    c = MT.case("lmc_D3_Q5")
    rows = []
    for mode in MODES:
        assert np.all(z[f"status{mode}"] == rounds) and np.all(z[f"pst{mode}"] == rounds), (z[f"status{mode}"], z[f"pst{mode}"])
        for i, p in enumerate(_CHILD_PS):
            got = {k: z[f"{k}{mode}"][i] for k in ("nlml", "grad", "dmean", "beta", "beta_cov")}
            rows += _hold(c, p, mode, got, f"jitter{rounds}", rounds, post=(z[f"pm{mode}_{i}"], z[f"pv{mode}_{i}"]))
    _assert_held(rows)


def test_theta_prior_is_added_as_in_nlml_grad():
    """a normal prior on every hyper of every slot: the new call's nlml and gradient move by what medgp_nlml_grad's move by (the same
    epilogue), to the rounding of the sums; dmean, beta and beta_cov keep their bits"""
    c = MT.case("lmc_D3_Q5")
    fam = MT.fam(c)
    ps = [1, 4]
    th = np.stack([c["th"][p] for p in ps])
    ctx = make_ctx(fam, [c["pts"][p] for p in ps], "pinned")
    H = th.shape[1]
    a0 = ctx.nlml_grad([0, 1], th, True)
    m0 = {mode: ctx.mean_nlml_grad([0, 1], th, **_kw(c, ps, mode)) for mode in MODES}
    for s in (0, 1):
        ctx.set_prior(s, np.ones(H, np.uint8), np.ones(H, np.int32), np.zeros(H, np.uint8), np.zeros(H, np.float32), np.ones(H, np.float32))
    a1 = ctx.nlml_grad([0, 1], th, True)
    m1 = {mode: ctx.mean_nlml_grad([0, 1], th, **_kw(c, ps, mode)) for mode in MODES}
    ctx.close()
    dn, dg = a1[0] - a0[0], a1[1] - a0[1]
    assert np.all(np.abs(dn) > 1) and np.any(dg != 0)
    for mode in MODES:
        for i in range(2):
            sn = max(abs(a1[0][i]), abs(m1[mode]["nlml"][i]), abs(dn[i]))
            assert abs((m1[mode]["nlml"][i] - m0[mode]["nlml"][i]) - dn[i]) <= 8 * 2.0 ** -53 * sn
            sg = np.maximum(np.maximum(np.abs(a1[1][i]), np.abs(m1[mode]["grad"][i])), np.abs(dg[i]))
            assert np.all(np.abs((m1[mode]["grad"][i] - m0[mode]["grad"][i]) - dg[i]) <= 8 * 2.0 ** -53 * sg)
            assert all(np.array_equal(_bits(m1[mode][k][i]), _bits(m0[mode][k][i])) for k in ("dmean", "beta", "beta_cov"))


def test_argument_and_capacity_errors():
    c = MT.case("lmc_D3_Q5")
    ctx = make_ctx(MT.fam(c), c["pts"])
    th = np.stack(c["th"])[:2]
    b0, lam = np.zeros((2, 3)), np.ones((2, 3))

    def code(fn):
        with pytest.raises(medgp_amd.MedgpError) as ei:
            fn()
        return int(str(ei.value).split("error ")[1].split(":")[0])
    for bad in (np.array([[1.0, -1.0, 1.0], [1, 1, 1]]), np.array([[1.0, np.nan, 1.0], [1, 1, 1]]), np.array([[1.0, np.inf, 1.0], [1, 1, 1]])):
        assert code(lambda: ctx.mean_nlml_grad([1, 2], th, b0, bad)) == -1
        assert code(lambda: ctx.mean_posterior([1, 2], th, [np.zeros(1, np.int32)] * 2, [np.zeros(1, np.float32)] * 2, b0, bad)) == -1
    assert code(lambda: ctx.mean_nlml_grad([1, 2], th, np.full((2, 3), np.nan), lam)) == -1
    import ctypes as C
    from medgp_amd.capi import _ptr
    sl, st = np.array([1, 2], np.int32), np.zeros(2, np.int32)
    nl = np.zeros(2)
    for mode in (-1, 2):   # a mode outside the two values
        assert ctx._lib.medgp_mean_nlml_grad(ctx._h, 2, _ptr(sl, C.c_int32), _ptr(th, C.c_double), mode, _ptr(b0, C.c_double), _ptr(lam, C.c_double), 1,
                                             _ptr(nl, C.c_double), None, None, None, None, _ptr(st, C.c_int32)) == -1
    assert ctx._lib.medgp_mean_nlml_grad(ctx._h, 2, _ptr(sl, C.c_int32), _ptr(th, C.c_double), 0, _ptr(b0, C.c_double), None, 1,
                                         _ptr(nl, C.c_double), None, None, None, None, _ptr(st, C.c_int32)) == -1   # MARGINAL without lam
    # every output pointer may be NULL
    assert ctx._lib.medgp_mean_nlml_grad(ctx._h, 2, _ptr(sl, C.c_int32), _ptr(th, C.c_double), 0, _ptr(b0, C.c_double), _ptr(lam, C.c_double), 1,
                                         None, None, None, None, None, None) == 0
    # the raw posterior call: the offset and NULL rules of the test points, refused before any device work (no launch, no allocation)
    m2, t2 = np.zeros(4, np.int32), np.linspace(1.0, 9.0, 4).astype(np.float32)
    mu, var, beta = np.zeros(4), np.zeros(4), np.zeros((2, 3))

    def raw(off, m2=m2, t2=t2, mu=mu, var=var):
        off = None if off is None else np.array(off, np.int64)
        return ctx._lib.medgp_mean_posterior_batch(ctx._h, 2, _ptr(sl, C.c_int32), _ptr(th, C.c_double), 0, _ptr(b0, C.c_double), _ptr(lam, C.c_double),
                                                   _ptr(off, C.c_int64), _ptr(m2, C.c_int32), _ptr(t2, C.c_float), _ptr(mu, C.c_double), _ptr(var, C.c_double),
                                                   _ptr(beta, C.c_double), _ptr(st, C.c_int32))
    assert raw([0, 1, 4]) == 0 and np.all(st == 0) and np.all(np.isfinite(mu)) and np.all(var > 0)
    ctx.profile_enable(True)
    ctx.profile_reset()
    allocs = ctx.alloc_stats()[1]
    assert raw([1, 1, 4]) == -1 and raw([0, 3, 2]) == -1                  # offsets[0] != 0; offsets that decrease
    assert raw(None) == -1 and raw([0, 1, 4], t2=None) == -1 and raw([0, 1, 4], m2=None) == -1
    assert raw([0, 1, 4], var=None) == -1 and raw([0, 1, 4], mu=None) == -1   # mean and var: both or neither
    assert raw([0, 1, 4], m2=np.array([0, 3, 0, 0], np.int32)) == -1      # a covariate outside [0, D)
    assert sum(v[1] for v in ctx.profile_read(all_entries=True).values()) == 0 and ctx.alloc_stats()[1] == allocs
    assert raw([0, 1, 4], mu=None, var=None) == 0                         # the per-point outputs may be NULL together
    ctx.profile_enable(False)
    r = ctx.mean_nlml_grad([1, 2], th, b0, lam)                           # the context stays usable
    assert np.all(r["status"] == 0) and np.all(np.isfinite(r["grad"]))
    ctx.close()
    # D = 65: the rank-D correction is one 64-column panel
    from medgp_amd import synth
    from random_patients import random_patient
    g = T._philox(20261721, 0)
    pt = random_patient(g, 65, 70, "plain")
    ctx = make_ctx((7, 1, 65, 1), [pt])
    th65 = synth.theta(4718, 0, 7, 1, 65, 1)[None]
    assert code(lambda: ctx.mean_nlml_grad([0], th65, np.zeros(65), np.ones(65))) == -4
    assert code(lambda: ctx.mean_posterior([0], th65, [np.zeros(1, np.int32)], [np.zeros(1, np.float32)], np.zeros(65), fixed=True)) == -4
    assert ctx.nlml_grad([0], th65, True)[2][0] == 0
    ctx.close()


def test_older_calls_keep_their_bits_behind_the_new_call():
    """nlml_grad, posterior and forecast on the same slots, called right behind the new calls, return the bits they returned before"""
    c = MT.case("lmc_D3_Q5")
    fam = MT.fam(c)
    P = len(c["pts"])
    th = np.stack(c["th"])
    sl = np.arange(P)
    m2l, t2l = _points(c, sl)
    ctx = make_ctx(fam, c["pts"], "pinned")

    def older():
        a = ctx.nlml_grad(sl, th, True)
        b, _ = ctx.posterior(sl, th, m2l, t2l)
        f, _ = ctx.forecast(sl, th, m2l, t2l)
        return a, b, f
    a0, b0_, f0 = older()
    for mode in MODES:
        ctx.mean_nlml_grad(sl, th, **_kw(c, sl, mode))
        a1, b1, f1 = older()
        ctx.mean_posterior(sl, th, m2l, t2l, **_kw(c, sl, mode))
        a2, b2, f2 = older()
        for a, b, f in ((a1, b1, f1), (a2, b2, f2)):
            # (patient 0 has n = 3 > 2: a status 0 everywhere)
            assert np.array_equal(_bits(a[0]), _bits(a0[0])) and np.array_equal(_bits(a[1]), _bits(a0[1])) and np.array_equal(a[2], a0[2])
            for i in range(P):
                for j in range(3):
                    assert np.array_equal(np.asarray(b[i][j]).view(np.uint32), np.asarray(b0_[i][j]).view(np.uint32)), (mode, i, j)
                for j in range(2):
                    assert np.array_equal(np.asarray(f[i][j]).view(np.uint32), np.asarray(f0[i][j]).view(np.uint32)), (mode, i, j)
    ctx.close()


def test_baseline_objective_closures():
    """medgp_amd.baseline.objective: the closures return the call's values; in the reference's layout the gradient is [grad | dmean]"""
    from medgp_amd import baseline
    c = MT.case("sm_Q3")
    ps = [1, 2]
    th = np.stack([c["th"][p] for p in ps])
    ctx = make_ctx(MT.fam(c), [c["pts"][p] for p in ps], "pinned")
    b0, lam = baseline.standard_prior(1)
    v, g = baseline.objective(ctx, [0, 1], b0, lam)(th)
    r = ctx.mean_nlml_grad([0, 1], th, b0, lam)
    assert np.array_equal(_bits(v), _bits(r["nlml"])) and np.array_equal(_bits(g), _bits(r["grad"]))
    mm = np.array([[0.25], [-0.5]])
    v2, g2 = baseline.objective(ctx, [0, 1], None, fixed=True, reference_layout=True)(baseline.reference_theta(th, mm))
    r2 = ctx.mean_nlml_grad([0, 1], th, mm, fixed=True)
    ctx.close()
    assert np.array_equal(_bits(v2), _bits(r2["nlml"])) and np.array_equal(_bits(g2), _bits(np.concatenate([r2["grad"], r2["dmean"]], axis=1)))
    db, dl = baseline.prior_grad(r["beta"], r["beta_cov"], b0, lam)
    assert np.array_equal(_bits(db), _bits(r["dmean"])) and np.all(np.isfinite(dl))
