"""medgp_set_basis / medgp_basis_nlml_grad / medgp_basis_posterior_batch on the MI355X against the long-double truth (basis_truth.py)
within the fp64 budget measured on CPU programs alone: every case of basis_truth (n = 3, 17, 63, 64, 65, 130, 200; p = 1, 2, 16, 17, 33,
64; SE, SM, LMC-SM with D = 3 and 24; trends, steps, ramps, harmonics, a dose column, dense bases; lam mixed per column including 0;
covariates interleaved) as one ragged batch in both modes on the default, the pinned and the look-ahead route; one jitter round; the
indicator basis against the baseline calls; bit invariance with the route pinned; the basis' lifecycle; argument and capacity
errors; the older calls' bits right behind the new calls; and no allocation across repeated evaluations."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
import basis_truth as BT
import mean_truth as MT
import nlml_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ["auto", "pinned", "la"]
MODES = [BT.MARGINAL, BT.FIXED]
MODE_NAME = {BT.MARGINAL: "marginal", BT.FIXED: "fixed"}
KEYS = ("nlml", "grad", "dbeta", "beta", "beta_cov")
X = np.longdouble


def make_ctx(fam, pts, Hs=None, route="auto", max_batch=None):
    kidx = fam[0]
    ctx = medgp_amd.Context(*fam)
    ctx.reserve(len(pts), max(max(p[1].shape[0] for p in pts), 1), max_batch or len(pts))
    for s, (m, t, y) in enumerate(pts):
        ctx.set_patient(s, m if kidx == 7 else None, t, y)
    if Hs is not None:
        ctx.set_basis(np.arange(len(pts)), Hs)
    if route == "pinned":
        ctx.pin_route(True)
    return ctx


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in KEYS if a[k] is not None)


def _kw(c, ps, mode):
    """the prior arguments of patients ps of a case"""
    b0 = np.stack([c["b0"][p] for p in ps])
    return dict(b0=b0, fixed=True) if mode == BT.FIXED else dict(b0=b0, lam=np.stack([c["lam"][p] for p in ps]))


def _points(c, ps):
    pp = [BT.points(c, p) for p in ps]
    return ([x[0] for x in pp] if c["kidx"] == 7 else None), [x[1] for x in pp], [x[2] for x in pp]


def _row(r, i):
    return {k: (None if r[k] is None else r[k][i]) for k in KEYS}


def _hold(c, p, mode, got, what, jitter_rounds=0, post=None):
    """one patient's device outputs against the truth within the budgets; prints error / budget per output"""
    tr, bud = BT.budget_of(c, p, mode, jitter_rounds)
    e = BT.errors(got, tr)
    if post is not None:
        e.update(BT.post_errors(post[0], post[1], tr["post"]))
    assert np.any(tr["grad"] != 0) and np.isfinite(float(tr["nlml"]))     # nothing passes against zeros
    rows = []
    for k, v in e.items():
        print(f"BASIS-ERR {what} {MODE_NAME[mode]} {c['id']}:{p} n {c['pts'][p][1].shape[0]} p {c['p']} {k}: {v:.3g} / {bud[k]:.3g}")
        rows.append((what, c["id"], p, k, v, bud[k]))
    return rows


def _assert_held(rows):
    bad = [r for r in rows if not r[4] <= r[5]]
    assert not bad, bad


_LEGS = [(s[0], r) for s in BT._SPECS for r in ROUTES if r != "la" or max(n for n, _ in s[7]) > 128]


@pytest.mark.parametrize("mode", MODES, ids=[MODE_NAME[m] for m in MODES])
@pytest.mark.parametrize("cid,route", _LEGS, ids=[f"{c}-{r}" for c, r in _LEGS])
def test_device_within_budget(cid, route, mode, monkeypatch):
    """every case as one ragged batch in a shuffled order: nlml, grad, dbeta, beta, beta_cov and the posterior within budget;
    flag_grad = 0 gives the same bits of what it returns"""
    c = BT.case(cid)
    P = len(c["pts"])
    if route == "la":
        monkeypatch.setenv("MEDGP_MULTI_CU", "1")
    order = np.roll(np.arange(P), 1)[::-1].copy()
    th = np.stack(c["th"])
    kw = _kw(c, order, mode)
    m2l, t2l, h2l = _points(c, order)
    ctx = make_ctx(BT.fam(c), c["pts"], c["H"], route)
    r = ctx.basis_nlml_grad(order, th[order], **kw)
    r0 = ctx.basis_nlml_grad(order, th[order], flag_grad=False, **kw)
    post, pbeta, pst = ctx.basis_posterior(order, th[order], m2l, t2l, h2l, **kw)
    ctx.close()
    rows = []
    for i, p in enumerate(order):
        tr = BT.truth_of(c, p, mode)
        assert r["status"][i] == tr["status"] == 0 and pst[i] == 0 and r0["status"][i] == 0, (p, r["status"], pst)
        assert r0["grad"] is None and all(np.array_equal(_bits(r0[k][i]), _bits(r[k][i])) for k in ("nlml", "dbeta", "beta", "beta_cov"))
        assert np.array_equal(_bits(pbeta[i]), _bits(r["beta"][i]))
        rows += _hold(c, p, mode, _row(r, i), route, post=post[i])
        if mode == BT.FIXED:
            assert np.array_equal(_bits(r["beta"][i]), _bits(c["b0"][p])) and not r["beta_cov"][i].any()
    _assert_held(rows)


def test_cases_span_two_size_classes():
    """the ragged batches above are cut into more than one size class (the plan of the call says so)"""
    c = BT.case("lmc_D3_p16")
    ctx = make_ctx(BT.fam(c), c["pts"], c["H"])
    ctx.basis_nlml_grad(np.arange(3), np.stack(c["th"]), **_kw(c, range(3), BT.MARGINAL))
    import ctypes as C
    cnt, blocks, route = (C.c_int32 * 8)(), (C.c_int32 * 8)(), (C.c_int32 * 8)()
    ncls = ctx._lib.medgp_last_plan(ctx._h, 8, cnt, blocks, route)
    ctx.close()
    assert ncls >= 2 and sum(cnt[:ncls]) == 3, (ncls, list(cnt))


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[2])
import basis_truth as BT
from test_basis_gpu import make_ctx, _kw, _points
c = BT.case("lmc_D3_p16")
ps = [0, 1, 2]
th = np.stack([c["th"][p] for p in ps])
ctx = make_ctx(BT.fam(c), c["pts"], c["H"], "pinned")
res = {}
for mode in (0, 1):
    r = ctx.basis_nlml_grad(np.arange(3), th, **_kw(c, ps, mode))
    m2l, t2l, h2l = _points(c, ps)
    post, _, pst = ctx.basis_posterior(np.arange(3), th, m2l, t2l, h2l, **_kw(c, ps, mode))
    res.update({f"{k}{mode}": r[k] for k in r})
    res[f"pst{mode}"] = pst
    for i in range(3):
        res[f"pm{mode}_{i}"], res[f"pv{mode}_{i}"] = post[i]
ctx.close()
np.savez(sys.argv[1], **res)
"""


def test_one_jitter_round(tmp_path):
    """every quantity is that of the matrix that was factored, K + diag(sigma^2); the hook is read when the library creates a
    context, in a process of its own"""
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), MEDGP_DEBUG_FAIL_ATTEMPTS="1")
    out = str(tmp_path / "jit.npz")
    pr = subprocess.run([sys.executable, "-c", _CHILD, out, os.path.join(ROOT, "tests")], env=e, capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr[-2000:]
    z = np.load(out)
    c = BT.case("lmc_D3_p16")
    rows = []
    for mode in MODES:
        assert np.all(z[f"status{mode}"] == 1) and np.all(z[f"pst{mode}"] == 1), (z[f"status{mode}"], z[f"pst{mode}"])
        for i in range(3):
            got = {k: z[f"{k}{mode}"][i] for k in KEYS}
            rows += _hold(c, i, mode, got, "jitter1", 1, post=(z[f"pm{mode}_{i}"], z[f"pv{mode}_{i}"]))
    _assert_held(rows)


def test_indicator_basis_agrees_with_the_baseline_calls():
    """H[i, d] = [m_i = d]: both families meet the same truth, so they agree within the sum of their two budgets (other kernels and
    summation orders: not bits), on the truth's own error scales"""
    worst = 0.0
    for cid in ("lmc_D3_Q5", "sm_Q3"):
        c = MT.case(cid)
        fam = MT.fam(c)
        P = len(c["pts"])
        ps = [p for p in range(P) if c["pts"][p][1].shape[0] > 3]
        pts = [c["pts"][p] for p in ps]
        th = np.stack([c["th"][p] for p in ps])
        Hs = [MT.hmat(c["kidx"], c["D"], m, t.shape[0], np.float64) for m, t, y in pts]
        pp = [MT.points(c, p) for p in ps]
        m2l, t2l = ([x[0] for x in pp] if c["kidx"] == 7 else None), [x[1] for x in pp]
        h2l = [MT.hmat(c["kidx"], c["D"], x[0], x[1].shape[0], np.float64) for x in pp]
        ctx = make_ctx(fam, pts, Hs)
        sl = np.arange(len(ps))
        for mode in MODES:
            b0 = np.stack([c["b0"][p] for p in ps])
            kw = dict(b0=b0, fixed=True) if mode == MT.FIXED else dict(b0=b0, lam=np.stack([c["lam"][p] for p in ps]))
            rb = ctx.basis_nlml_grad(sl, th, **kw)
            rm = ctx.mean_nlml_grad(sl, th, **kw)
            pb, _, stb = ctx.basis_posterior(sl, th, m2l, t2l, h2l, **kw)
            pm, _, stm = ctx.mean_posterior(sl, th, m2l, t2l, **kw)
            for i, p in enumerate(ps):
                assert rb["status"][i] == rm["status"][i] == stb[i] == stm[i] == 0
                trm, budm = MT.budget_of(c, p, mode)
                lam_p = None if mode == MT.FIXED else c["lam"][p]
                prb = BT.programs_for(c, p, mode, Hs[i], c["b0"][p], lam_p, 0, (pp[i][0], pp[i][1], h2l[i]))
                budb, trb = BT.budgets(prb), prb["truth"]
                pairs = [("nlml", rb["nlml"][i], rm["nlml"][i], trb["nlml_mag"], "nlml"), ("grad", rb["grad"][i], rm["grad"][i], np.abs(trb["grad"]), "grad"),
                         ("dbeta", rb["dbeta"][i], rm["dmean"][i], trb["dbeta_mag"], "dmean"), ("beta", rb["beta"][i], rm["beta"][i], np.abs(trb["beta"]), "beta"),
                         ("beta_cov", rb["beta_cov"][i], rm["beta_cov"][i], np.abs(trb["beta_cov"]), "beta_cov"),
                         ("mean", pb[i][0], pm[i][0], trb["post"]["mag_mean"], "mean"), ("var", pb[i][1], pm[i][1], trb["post"]["mag_var"], "var")]
                for kb, a, b, mag, km in pairs:
                    d = BT.error_of(a, np.asarray(b, X), mag)
                    lim = budb[kb] + budm[km]
                    print(f"BASIS-ERR indicator {MODE_NAME[mode]} {cid}:{p} {kb}: {d:.3g} / {lim:.3g}")
                    worst = max(worst, d / lim)
                    assert d <= lim, (cid, p, mode, kb, d, lim)
        ctx.close()
    print(f"BASIS-ERR indicator worst fraction of the summed budgets: {worst:.3g}")


def _singular_setup():
    """case lmc_D3_p16 in four slots: 0..2 its patients, 3 patient 1 again with column 15 a copy of column 0 -- under lam_0 = lam_15 = 0
    a dependent flat-prior pair"""
    c = BT.case("lmc_D3_p16")
    Hd = c["H"][1].copy()
    Hd[:, 15] = Hd[:, 0]
    pts = list(c["pts"]) + [c["pts"][1]]
    Hs = list(c["H"]) + [Hd]
    return c, pts, Hs


def test_bit_invariance_with_the_route_pinned():
    """an entry's bits depend on its own operands alone: alone, in a batch of 7, reversed, at another position, beside a singular-A
    entry and a failed factorisation; a point's not on the other points or their order; a patient may have no points"""
    c, pts, Hs = _singular_setup()
    ctx = make_ctx(BT.fam(c), pts, Hs, "pinned", max_batch=7)
    for mode in MODES:
        batch = [2, 1, 0, 2, 1, 0, 1]
        th = np.stack([c["th"][p] for p in batch])
        m2l, t2l, h2l = _points(c, batch)
        full = ctx.basis_nlml_grad(batch, th, **_kw(c, batch, mode))
        fpost, _, fst = ctx.basis_posterior(batch, th, m2l, t2l, h2l, **_kw(c, batch, mode))
        rev = ctx.basis_nlml_grad(batch[::-1], th[::-1], **_kw(c, batch[::-1], mode))
        assert np.all(full["status"] == 0) and np.all(fst == 0)
        assert _same(_row(full, 0), _row(full, 3)) and _same(_row(full, 1), _row(full, 6))   # another position
        for i, p in enumerate(batch):
            assert _same(_row(rev, 6 - i), _row(full, i)), (mode, i)
        for i, p in enumerate(batch[:3]):
            one = ctx.basis_nlml_grad([p], th[i:i + 1], **_kw(c, [p], mode))
            assert _same(_row(one, 0), _row(full, i)), (mode, i)
        # the points of patient 2 reversed and alone; patient 1 beside it without points
        z = np.zeros(0)
        pr, _, pst = ctx.basis_posterior([2, 1], th[:2], None if m2l is None else [m2l[0][::-1].copy(), z.astype(np.int32)],
                                         [t2l[0][::-1].copy(), z.astype(np.float32)], [h2l[0][::-1].copy(), np.zeros((0, c["p"]))], **_kw(c, [2, 1], mode))
        assert np.array_equal(_bits(pr[0][0][::-1]), _bits(fpost[0][0])) and np.array_equal(_bits(pr[0][1][::-1]), _bits(fpost[0][1]))
        assert pr[1][0].shape == (0,) and list(pst) == [0, 0]
    # beside a singular-A entry (slot 3, MARGINAL with the pair flat) and a failed factorisation (NaN theta)
    batch = [0, 3, 1, 2]
    ps = [0, 1, 1, 2]
    th = np.stack([c["th"][p] for p in ps])
    kw = _kw(c, ps, BT.MARGINAL)
    kw["lam"] = kw["lam"].copy()
    kw["lam"][1, [0, 15]] = 0.0
    m2l, t2l, h2l = _points(c, ps)
    thf = th.copy()
    thf[2, 0] = np.nan
    good = ctx.basis_nlml_grad([0, 2], th[[0, 3]], b0=kw["b0"][[0, 3]], lam=kw["lam"][[0, 3]])
    gpost, _, _ = ctx.basis_posterior([0, 2], th[[0, 3]], [m2l[0], m2l[3]], [t2l[0], t2l[3]], [h2l[0], h2l[3]], b0=kw["b0"][[0, 3]], lam=kw["lam"][[0, 3]])
    r = ctx.basis_nlml_grad(batch, thf, **kw)
    post, pbeta, pst = ctx.basis_posterior(batch, thf, m2l, t2l, h2l, **kw)
    rf = ctx.basis_nlml_grad(batch, thf, b0=kw["b0"], fixed=True)        # FIXED ignores lam: the pair is harmless there
    ctx.close()
    assert list(r["status"]) == [0, -1, -1, 0] and list(pst) == [0, -1, -1, 0] and list(rf["status"]) == [0, 0, -1, 0]
    for i in (1, 2):
        assert all(np.all(np.isnan(r[k][i])) for k in KEYS), i
        assert np.all(np.isnan(post[i][0])) and np.all(np.isnan(post[i][1])) and np.all(np.isnan(pbeta[i]))
    for i, j in ((0, 0), (3, 1)):
        assert all(np.all(np.isfinite(r[k][i])) for k in KEYS)
        assert _same(_row(r, i), _row(good, j)), i
        assert np.array_equal(_bits(post[i][0]), _bits(gpost[j][0])) and np.array_equal(_bits(post[i][1]), _bits(gpost[j][1]))
    assert np.all(np.isfinite(rf["grad"][1])) and np.all(np.isnan(rf["grad"][2]))


def test_older_calls_keep_their_bits_behind_the_new_calls():
    """nlml_grad, mean_nlml_grad and posterior on the same slots, called right behind the new calls, return the bits they returned
    before them"""
    c = BT.case("lmc_D3_p16")
    P = len(c["pts"])
    th = np.stack(c["th"])
    sl = np.arange(P)
    m2l, t2l, h2l = _points(c, sl)
    ctx = make_ctx(BT.fam(c), c["pts"], c["H"], "pinned")
    b0m, lamm = np.array([0.1, -0.2, 0.3]), np.array([1.0, 0.0, 0.05])

    def older():
        a = ctx.nlml_grad(sl, th, True)
        mm = ctx.mean_nlml_grad(sl, th, b0m, lamm)
        b, _ = ctx.posterior(sl, th, m2l, t2l)
        return a, mm, b
    a0, mm0, b0_ = older()
    for mode in MODES:
        ctx.basis_nlml_grad(sl, th, **_kw(c, sl, mode))
        got = [older()]
        ctx.basis_posterior(sl, th, m2l, t2l, h2l, **_kw(c, sl, mode))
        got.append(older())
        for a, mm, b in got:
            assert np.array_equal(_bits(a[0]), _bits(a0[0])) and np.array_equal(_bits(a[1]), _bits(a0[1])) and np.array_equal(a[2], a0[2])
            assert all(np.array_equal(_bits(mm[k]), _bits(mm0[k])) for k in ("nlml", "grad", "dmean", "beta", "beta_cov"))
            for i in range(P):
                for j in range(3):
                    assert np.array_equal(np.asarray(b[i][j]).view(np.uint32), np.asarray(b0_[i][j]).view(np.uint32)), (mode, i, j)
    ctx.close()


def _code(fn):
    with pytest.raises(medgp_amd.MedgpError) as ei:
        fn()
    return int(str(ei.value).split("error ")[1].split(":")[0])


def test_basis_lifecycle_and_argument_errors():
    c = BT.case("lmc_D3_p16")
    ctx = make_ctx(BT.fam(c), c["pts"], None, "pinned")
    th = np.stack(c["th"])
    sl = np.arange(3)
    kw = _kw(c, sl, BT.MARGINAL)
    m2l, t2l, h2l = _points(c, sl)
    assert _code(lambda: ctx.basis_nlml_grad(sl, th, **kw)) == -1                        # no basis yet
    ctx.set_basis(sl, c["H"])
    r1 = ctx.basis_nlml_grad(sl, th, **kw)
    # set_basis twice replaces the basis: other rows, other results; the first rows again, the first bits again
    H2 = [h * 0.5 for h in c["H"]]
    ctx.set_basis(sl, H2)
    r2 = ctx.basis_nlml_grad(sl, th, **kw)
    assert np.all(r2["status"] == 0) and not np.array_equal(_bits(r2["nlml"]), _bits(r1["nlml"]))
    ctx.set_basis([2, 0], [c["H"][2], c["H"][0]])                                         # another order, a subset: placed elsewhere
    ctx.set_basis([1], [c["H"][1]])
    r3 = ctx.basis_nlml_grad(sl, th, **kw)
    assert _same(r3, r1)
    # mixed p in one call
    ctx.set_basis([1], [c["H"][1][:, :7]])
    assert _code(lambda: ctx.basis_nlml_grad(sl, th, **kw)) == -1
    r7 = ctx.basis_nlml_grad([1], th[1:2], b0=np.zeros(7), lam=np.ones(7))
    assert r7["status"][0] == 0 and r7["beta_cov"].shape == (1, 7, 7)
    ctx.set_basis([1], [c["H"][1]])
    # NULL removes it; set_patient drops it
    ctx.set_basis([0], None)
    assert _code(lambda: ctx.basis_nlml_grad(sl, th, **kw)) == -1
    assert _code(lambda: ctx.basis_posterior(sl, th, m2l, t2l, h2l, **kw)) == -1
    ctx.set_basis([0], [c["H"][0]])
    assert _same(ctx.basis_nlml_grad(sl, th, **kw), r1)
    ctx.set_patient(2, *c["pts"][2])
    assert _code(lambda: ctx.basis_nlml_grad(sl, th, **kw)) == -1
    assert _same(ctx.basis_nlml_grad([0, 1], th[:2], b0=kw["b0"][:2], lam=kw["lam"][:2]), {k: r1[k][:2] for k in r1})
    ctx.set_basis([2], [c["H"][2]])
    # argument errors of set_basis
    assert _code(lambda: ctx.set_basis([0], [np.zeros((c["H"][0].shape[0], 65))])) == -4           # p = 65: capacity
    assert _code(lambda: ctx.set_basis([0], [np.zeros((c["H"][0].shape[0], 0))])) == -1            # p = 0
    bad = c["H"][0].copy()
    bad[5, 3] = np.nan
    assert _code(lambda: ctx.set_basis([0], [bad])) == -1
    bad[5, 3] = np.inf
    assert _code(lambda: ctx.set_basis([0], [bad])) == -1
    assert _code(lambda: ctx.set_basis([0], [c["H"][0][:-1]])) == -1                               # a row count that is not n
    assert _code(lambda: ctx.set_basis([0, 0], [c["H"][0], c["H"][0]])) == -1                      # a duplicate slot
    assert _same(ctx.basis_nlml_grad(sl, th, **kw), r1)                                            # nothing was changed by the refused calls
    # h2: required, finite
    hb = [h.copy() for h in h2l]
    hb[1][2, 4] = np.nan
    assert _code(lambda: ctx.basis_posterior(sl, th, m2l, t2l, hb, **kw)) == -1
    import ctypes as C
    from medgp_amd.capi import _ptr
    sl32, st = sl.astype(np.int32), np.zeros(3, np.int32)
    off = np.array([0, 1, 1, 1], np.int64)
    mm, tt = np.zeros(1, np.int32), np.zeros(1, np.float32)
    assert ctx._lib.medgp_basis_posterior_batch(ctx._h, 3, _ptr(sl32, C.c_int32), _ptr(th, C.c_double), 0, _ptr(kw["b0"], C.c_double), _ptr(kw["lam"], C.c_double),
                                                off.ctypes.data_as(C.POINTER(C.c_int64)), _ptr(mm, C.c_int32), _ptr(tt, C.c_float), None, None, None, None,
                                                _ptr(st, C.c_int32)) == -1
    # the mean calls' argument errors; every output pointer may be NULL
    assert _code(lambda: ctx.basis_nlml_grad(sl, th, kw["b0"], -kw["lam"] - 1)) == -1
    assert _code(lambda: ctx.basis_nlml_grad(sl, th, np.full((3, 16), np.nan), kw["lam"])) == -1
    assert ctx._lib.medgp_basis_nlml_grad(ctx._h, 3, _ptr(sl32, C.c_int32), _ptr(th, C.c_double), 2, _ptr(kw["b0"], C.c_double), _ptr(kw["lam"], C.c_double), 1,
                                          None, None, None, None, None, None) == -1
    assert ctx._lib.medgp_basis_nlml_grad(ctx._h, 3, _ptr(sl32, C.c_int32), _ptr(th, C.c_double), 0, _ptr(kw["b0"], C.c_double), _ptr(kw["lam"], C.c_double), 1,
                                          None, None, None, None, None, None) == 0
    # an empty slot
    ctx2 = medgp_amd.Context(*BT.fam(c))
    ctx2.reserve(2, 64, 2)
    assert _code(lambda: ctx2.set_basis([0], [np.zeros((3, 2))])) == -1
    ctx2.close()
    ctx.close()


def test_dependent_flat_pair_is_status_minus_one_and_a_zero_column_is_legal():
    c, pts, Hs = _singular_setup()
    Hz = c["H"][1].copy()
    Hz[:, 15] = 0.0
    Hs = Hs[:3] + [Hs[3], Hz]
    pts = pts + [c["pts"][1]]
    ctx = make_ctx(BT.fam(c), pts, Hs, "pinned")
    ps = [0, 1, 2, 1, 1]
    th = np.stack([c["th"][p] for p in ps])
    kw = _kw(c, ps, BT.MARGINAL)
    lam = kw["lam"].copy()
    lam[3, [0, 15]] = 0.0          # slot 3: the dependent pair, both flat
    lam[4, 15] = 0.05              # slot 4: a zero column under a proper prior
    r = ctx.basis_nlml_grad(np.arange(5), th, kw["b0"], lam)
    lam[4, 15] = 0.0               # ... and under the flat prior: nothing determines it
    rz = ctx.basis_nlml_grad(np.arange(5), th, kw["b0"], lam)
    ctx.close()
    assert list(r["status"]) == [0, 0, 0, -1, 0] and list(rz["status"]) == [0, 0, 0, -1, -1]
    assert all(np.all(np.isfinite(r[k][i])) for k in KEYS for i in (0, 1, 2, 4)) and all(np.all(np.isnan(r[k][3])) for k in KEYS)
    assert r["beta"][4, 15] == kw["b0"][4, 15] and r["dbeta"][4, 15] == 0
    assert abs(r["beta_cov"][4, 15, 15] * 0.05 - 1) <= 1e-15 and not np.delete(r["beta_cov"][4, 15], 15).any()
    tr = BT.woodbury(*BT.fam(c), *c["pts"][1], c["th"][1], Hs[3], BT.MARGINAL, kw["b0"][3], lam[3], X)
    assert tr["status"] == -1


def test_no_allocation_across_repeated_evaluations():
    """after set_basis and one warm-up of each call the evaluations obtain no memory: medgp_alloc_stats does not move"""
    c = BT.case("lmc_D3_p16")
    ctx = make_ctx(BT.fam(c), c["pts"], c["H"], "pinned")
    th = np.stack(c["th"])
    sl = np.arange(3)
    m2l, t2l, h2l = _points(c, sl)
    import ctypes as C

    def stats():
        s, n, b = C.c_double(), C.c_int64(), C.c_int64()
        assert ctx._lib.medgp_alloc_stats(ctx._h, C.byref(s), C.byref(n), C.byref(b)) == 0
        return n.value, b.value
    for mode in MODES:
        ctx.basis_nlml_grad(sl, th, **_kw(c, sl, mode))
        ctx.basis_posterior(sl, th, m2l, t2l, h2l, **_kw(c, sl, mode))
    s0 = stats()
    for _ in range(3):
        ctx.set_basis(sl, c["H"])          # the training loop's repeat: in place
        for mode in MODES:
            ctx.basis_nlml_grad(sl, th, **_kw(c, sl, mode))
            ctx.basis_posterior(sl, th, m2l, t2l, h2l, **_kw(c, sl, mode))
    assert stats() == s0
    ctx.close()
