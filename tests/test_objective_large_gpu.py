"""medgp_loo_grad, medgp_lgo_grad, medgp_forecast_grad and medgp_fisher_vec on the MI355X above N = 512 (objective_large.py): every
leg of the large sweep -- second passes of the factorisation (n = 513 .. 1024, alone and as one ragged batch), the Q > 8 split
(Q = 8, 9, 16 at n = 640), D = 64, the single-output families at n = 1024, and n = 2048 with the z history out of LDS -- against the
committed long-double truths within the fp64 budgets measured on CPU programs alone, on the default routing, the pinned
one-workgroup route and the look-ahead route (MEDGP_MULTI_CU=1, read when the context is created).  All four calls run the shared
factorisation pipeline, whose route decides which kernels leave alpha, P and U behind, so the look-ahead route is run for every
objective.  Then: bit invariance at size, relabelled group ids, flag_grad = 0, the group limit of the leave-group-out blocks and
the Q > 16 refusal.  Every truth comes from tests/golden/objective_truth_large.npz; nothing slow is recomputed here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
import nlml_truth as T
import objective_large as OL

ROUTES = ["auto", "pinned", "la"]


def make_ctx(fam, pts, route, monkeypatch):
    if route == "la":
        monkeypatch.setenv("MEDGP_MULTI_CU", "1")
    kidx = fam[0]
    ctx = medgp_amd.Context(*fam)
    ctx.reserve(len(pts), max(p[1].shape[0] for p in pts), len(pts))
    for s, (m, t, y) in enumerate(pts):
        ctx.set_patient(s, m if kidx == 7 else None, t, y)
    if route == "pinned":
        ctx.pin_route(True)
    return ctx


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def call(ctx, obj, slots, th, tabs, flag=True):
    """one call of objective obj on the slots with one table per slot: (objective values or None, gradients / products, status)"""
    if obj == "loo":
        return ctx.loo_grad(slots, th, flag)
    if obj == "lgo":
        o, g, st, gst = ctx.lgo_grad(slots, th, [tb[0] for tb in tabs], flag)
        assert all(np.all(x == 0) for x in gst), gst
        return o, g, st
    if obj == "fc":
        return ctx.forecast_grad(slots, th, tabs, int(flag))
    fv, st = ctx.fisher_vec(slots, th, np.stack(tabs))
    return None, fv, st


def _hold(e, o, g, what):
    """one entry's device output against its committed truth within its budget; prints the observed errors beside the budgets"""
    tj, tg, bj, bg = OL.budgets(e)
    ej, eg = OL.errors_of(e, (o, g), (tj, tg))
    oj = "" if ej is None else f"obj {ej:.3g} (budget {bj:.3g}, {ej / bj:.2f}), "
    print(f"OBJLARGE-ERR {what} {OL.key_of(e)} n {OL.n_of(e[1], e[2])}: {oj}grad {eg:.3g} (budget {bg:.3g}, {eg / bg:.2f})")
    return (what, OL.key_of(e), ej, bj, eg, bg)


def _assert_held(rows):
    assert rows
    bad = [r for r in rows if not (r[4] <= r[5] and (r[2] is None or r[2] <= r[3]))]
    assert not bad, bad


_ENV_TABLES = {"cap960"}       # run under a budget of their own: test_group_limit
_UNITS = sorted({(e[0], e[1], e[3]) for e in OL.entries()}, key=lambda u: (OL.CASE_ORDER.index(u[1]), OL.OBJECTIVES.index(u[2])))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("leg,cid,obj", _UNITS, ids=[f"{u[0]}-{u[1]}-{u[2]}" for u in _UNITS])
def test_device_within_budget(leg, cid, obj, route, monkeypatch):
    """every entry of one case and objective: each patient alone under each of its tables, then (leg pass2) the four patients as one
    ragged batch under every table all four have.  Rows are collected, then asserted once."""
    es = [e for e in OL.entries(leg, obj) if e[1] == cid and e[4] not in _ENV_TABLES]
    c = OL.case(cid, obj)
    P = len(c["pts"])
    th = np.stack(c["th"])
    ctx = make_ctx(OL.fam(c), c["pts"], route, monkeypatch)
    rows = []
    for e in es:
        p = e[2]
        o, g, st = call(ctx, obj, [p], th[p:p + 1], [OL.table_of(e)])
        assert st[0] == 0, (e, st)
        rows.append(_hold(e, None if o is None else o[0], g[0], f"{route} alone"))
    if P > 1:
        order = np.array([2, 0, 3, 1])
        for tab in sorted({e[4] for e in es}):
            be = {e[2]: e for e in es if e[4] == tab}
            if len(be) < P:
                continue
            o, g, st = call(ctx, obj, order, th[order], [OL.table_of(be[p]) for p in order])
            assert np.all(st == 0), (tab, st)
            for i, p in enumerate(order):
                rows.append(_hold(be[p], None if o is None else o[i], g[i], f"{route} ragged"))
    ctx.close()
    _assert_held(rows)


_BIT_TABLES = {"loo": "-", "lgo": "cov", "fc": "h48", "fisher": "v2"}


@pytest.mark.parametrize("obj", OL.OBJECTIVES)
def test_bits_alone_and_in_the_ragged_batch(obj, monkeypatch):
    """pinned route: the n = 768 patient's objective and gradient (or products) alone have the bits they have inside the ragged
    batch of four, in both batch orders"""
    c = OL.case("large_pass2", obj)
    th = np.stack(c["th"])
    tabs = [OL.table_of(("pass2", "large_pass2", p, obj, _BIT_TABLES[obj])) for p in range(4)]
    ctx = make_ctx(OL.fam(c), c["pts"], "pinned", monkeypatch)
    ao, ag, st = call(ctx, obj, [2], th[2:3], [tabs[2]])
    assert st[0] == 0 and c["pts"][2][1].shape[0] == 768
    for order in (np.arange(4), np.arange(4)[::-1].copy()):
        o, g, st = call(ctx, obj, order, th[order], [tabs[p] for p in order])
        i = int(np.flatnonzero(order == 2)[0])
        assert np.all(st == 0)
        assert np.array_equal(_bits(g[i]), _bits(ag[0])), (obj, list(order))
        assert o is None or _bits(o)[i] == _bits(ao)[0], (obj, list(order))
    ctx.close()


@pytest.mark.parametrize("route", ["auto", "pinned"])
def test_relabelled_groups_give_the_same_bits(route, monkeypatch):
    """table (a), two interleaved groups of 320 at n = 640, Q = 9: the same partition under other labels (the two ids swapped; ids
    3 and 1 of five) gives the same bits"""
    e = ("qsplit", "large_q_Q9", 0, "lgo", "two320")
    c = OL.case(e[1], "lgo")
    g, ng = OL.table_of(e)
    th = c["th"][0][None, :]
    ctx = make_ctx(OL.fam(c), c["pts"], route, monkeypatch)
    o, gr, st = call(ctx, "lgo", [0], th, [(g, ng)])
    for lab in ((1, 0), (3, 1)):
        o2, gr2, st2 = call(ctx, "lgo", [0], th, [(np.array(lab, np.int32)[g], max(lab) + 1)])
        assert st[0] == 0 and st2[0] == 0
        assert np.array_equal(_bits(o2), _bits(o)) and np.array_equal(_bits(gr2), _bits(gr)), lab
    ctx.close()
    _assert_held([_hold(e, o[0], gr[0], f"{route} relabel base")])


@pytest.mark.parametrize("cid,obj,tab", [("large_pass2", "loo", "-"), ("large_pass2", "lgo", "cov"), ("large_pass2", "lgo", "max"),
                                         ("large_pass2", "fc", "h48"), ("large_sm_Q4", "loo", "-"), ("large_sm_Q4", "fc", "h48")])
def test_objective_only_call_has_the_same_bits(cid, obj, tab, monkeypatch):
    """flag_grad = 0 at n = 1024: the objective has the bits it has with the gradient"""
    p = len(OL.base_case(cid)["pts"]) - 1
    assert OL.n_of(cid, p) == 1024
    c = OL.case(cid, obj)
    tb = OL.table_of((None, cid, p, obj, tab))
    th = c["th"][p][None, :]
    ctx = make_ctx(OL.fam(c), [c["pts"][p]], "auto", monkeypatch)
    o1, g1, st1 = call(ctx, obj, [0], th, [tb])
    o0, g0, st0 = call(ctx, obj, [0], th, [tb], False)
    ctx.close()
    assert st1[0] == 0 and st0[0] == 0 and g0 is None and g1 is not None
    assert np.array_equal(_bits(o0), _bits(o1)), (o0, o1)


@pytest.mark.parametrize("route", ROUTES)
def test_group_limit(route, monkeypatch):
    """the leave-group-out block limit (inference_tables.h, build_loo_tables).  The default budget of 2 GiB admits 11584 rows, more
    than any patient here: its largest group at n = 1024 is the whole patient (table "max", held in test_device_within_budget).
    Under MEDGP_POSTERIOR_BUDGET_GB = 15 MiB the limit is 960 rows: 960 in one group and 64 singletons are held to the budget, one
    row more is MEDGP_ERR_CAPACITY.  (The budget is read when the context is created.)"""
    monkeypatch.setenv("MEDGP_POSTERIOR_BUDGET_GB", repr(OL.CAP_BUDGET_GB))
    e = ("pass2", "large_pass2", 3, "lgo", "cap960")
    c = OL.case(e[1], "lgo")
    th = c["th"][3][None, :]
    ctx = make_ctx(OL.fam(c), [c["pts"][3]], route, monkeypatch)
    g, ng = OL.table_of(e)
    assert np.bincount(g).max() == 960
    o, gr, st = call(ctx, "lgo", [0], th, [(g, ng)])
    assert st[0] == 0
    g1, ng1 = OL.one_past(e[1], 3, "cap960")
    assert np.bincount(g1).max() == 961
    with pytest.raises(medgp_amd.MedgpError) as err:
        ctx.lgo_grad([0], th, [g1])
    assert "MEDGP_POSTERIOR_BUDGET_GB" in str(err.value) and "-4" in str(err.value) and "961" in str(err.value)   # MEDGP_ERR_CAPACITY
    o2, gr2, st2 = call(ctx, "lgo", [0], th, [(g, ng)])          # the context is still usable, and gives the same bits
    ctx.close()
    assert st2[0] == 0 and np.array_equal(_bits(o2), _bits(o)) and np.array_equal(_bits(gr2), _bits(gr))
    _assert_held([_hold(e, o[0], gr[0], f"{route} limit")])


def test_q17_is_refused_by_every_call(monkeypatch):
    """the calls keep K^-1 (Qm) where the generic gradient route keeps W: a Q = 17 context gets MEDGP_ERR_ARG from each"""
    c = [x for x in T.large_cases() if x["id"] == "large_q_Q17"][0]
    assert c["Q"] == 17 and c["pts"][0][1].shape[0] == 640
    th = c["th"][0][None, :]
    ctx = make_ctx(OL.fam(c), c["pts"], "auto", monkeypatch)
    calls = {"medgp_loo_grad": lambda: ctx.loo_grad([0], th),
             "medgp_lgo_grad": lambda: ctx.lgo_grad([0], th, [np.zeros(640, np.int32)]),
             "medgp_forecast_grad": lambda: ctx.forecast_grad([0], th, None),
             "medgp_fisher_vec": lambda: ctx.fisher_vec([0], th, np.ones_like(th))}
    for name, f in calls.items():
        with pytest.raises(medgp_amd.MedgpError) as err:
            f()
        assert "error -1" in str(err.value) and name in str(err.value) and "Q <= 16" in str(err.value), (name, str(err.value))
    nl, gr, st = ctx.nlml_grad([0], th, True)                     # the context is usable, and medgp_nlml_grad takes Q = 17
    ctx.close()
    assert st[0] == 0 and np.isfinite(nl[0])


def test_one_group_is_the_nlml_gradient_on_the_device(monkeypatch):
    """table (b): one group of all 576 observations is the nlml without a prior.  medgp_lgo_grad and medgp_nlml_grad of the same
    context agree within the sum of the two budgets, each output's error measured against the other call's output on the truth's
    scale.  The nlml budget is nlml_truth's rule on its two numpy fp64 programs, measured against the entry's committed truth
    (tests/test_objective_large.py holds that truth to nlml_truth's own long-double value)."""
    e = ("pass2", "large_pass2", 1, "lgo", "one")
    c = OL.case(e[1], "lgo")
    m, t, y = c["pts"][1]
    tj, tg, bj, bg = OL.budgets(e)
    en = [T.error_pair(*T.nlml_grad(*OL.fam(c), m, t, y, c["th"][1], np.float64, variant=v)[1:], tj, tg) for v in ("plain", "device")]
    bn, bgn = T.budget([x[0] for x in en], T.M_NLML), T.budget([x[1] for x in en], T.M_GRAD)
    th = c["th"][1][None, :]
    ctx = make_ctx(OL.fam(c), [c["pts"][1]], "auto", monkeypatch)
    o, g, st = call(ctx, "lgo", [0], th, [OL.table_of(e)])
    nl, gn, nst = ctx.nlml_grad([0], th, True)
    ctx.close()
    assert st[0] == 0 and nst[0] == 0
    dj, dg = T.error_pair(o[0], g[0], np.longdouble(nl[0]), gn[0].astype(np.longdouble))
    print(f"OBJLARGE-ERR one group against nlml_grad n 576: obj {dj:.3g} (bound {bj + bn:.3g}), grad {dg:.3g} (bound {bg + bgn:.3g})")
    assert dj <= bj + bn and dg <= bg + bgn
    _assert_held([_hold(e, o[0], g[0], "one group")])
