"""medgp_forecast_grad on the MI355X: objective and gradient against the long-double refit truth (forecast_grad_truth.py) within the
fp64 budget measured on CPU programs alone -- every size at which the kernels take another path, every family, both factorisation
routes, horizons 0 h and 6 h, patients uploaded in time order with interleaved covariates; agreement with medgp_forecast_batch and
(full histories) with medgp_nlml_grad; upload order; bit invariance; jitter retries; a failed patient; priors; argument errors; and
that the calls before and after it are not disturbed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
from medgp_amd import forecast, synth
import forecast_grad_truth as F
import forecast_ref as FR
import loo_grad_truth as G
import nlml_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ["auto", "pinned"]


def make_ctx(fam, pts, route="auto"):
    kidx = fam[0]
    ctx = medgp_amd.Context(*fam)
    ctx.reserve(len(pts), max(max(p[1].shape[0] for p in pts), 1), len(pts))
    for s, (m, t, y) in enumerate(pts):
        ctx.set_patient(s, m if kidx == 7 else None, t, y)
    if route == "pinned":
        ctx.pin_route(True)
    return ctx


def _hold(c, p, pf, obj, grad, what, jitter_rounds=0):
    """one patient's device output against the truth within the budget; prints the observed errors beside the budgets"""
    tj, tg, bj, bg = F.budget_of(c, p, pf, jitter_rounds)
    ej, eg = F.error_pair(obj, grad, tj, tg)
    print(f"FCGRAD-ERR {what} {c['id']}:{p} n {c['pts'][p][1].shape[0]}: obj {ej:.3g} (budget {bj:.3g}, {ej / bj:.2f}), grad {eg:.3g} (budget {bg:.3g}, {eg / bg:.2f})")
    return (what, c["id"], p, ej, bj, eg, bg)


def _assert_held(rows):
    bad = [r for r in rows if not (r[3] <= r[4] and r[5] <= r[6])]
    assert not bad, bad


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("cid", F.CASE_IDS)
def test_device_within_budget(cid, route):
    """every patient of the case alone, then (more than one patient) the ragged call mixing all sizes; both horizons"""
    c = F.case(cid)
    P = len(c["pts"])
    th = np.stack(c["th"])
    ctx = make_ctx(F.fam(c), c["pts"], route)
    rows = []
    for h in F.HORIZONS:
        pfs = [F.prefix_of(c, p, h) for p in range(P)]
        for p in range(P):
            obj, grad, st = ctx.forecast_grad([p], th[p:p + 1], [pfs[p]])
            assert st[0] == 0, (p, st)
            rows.append(_hold(c, p, pfs[p], obj[0], grad[0], f"{route} {h:g}h alone"))
        if P > 1:
            order = np.array([5, 0, 3, 6, 1, 4, 2])
            obj, grad, st = ctx.forecast_grad(order, th[order], [pfs[p] for p in order])
            assert np.all(st == 0), st
            for i, p in enumerate(order):
                rows.append(_hold(c, p, pfs[p], obj[i], grad[i], f"{route} {h:g}h ragged"))
    ctx.close()
    _assert_held(rows)


def _band_tables(n):
    """prefix tables whose bands [p_i, i] sit inside one 64-block, end on a block edge and span three blocks (n >= 130)"""
    i = np.arange(n)
    inside = np.maximum(i - (i % 64) // 2, 0)                   # p_i in the block of i
    edge = np.where(i >= 64, (i // 64) * 64, i)                 # the band starts on the edge of the block of i
    three = np.where(i >= 128, np.minimum(i - 128, 5), -1)      # rows of the third block and later: bands over >= three blocks
    return {"inside": inside, "edge": edge, "three_blocks": three}


@pytest.mark.parametrize("route", ROUTES)
def test_band_shapes_and_degenerate_tables(route):
    """n = 130 and 200 under bands of every shape, nothing scored, the prior predictive (prefix 0) and the last observation alone"""
    c = F.case("lmc_sizes")
    ps = [5, 6]
    th = np.stack([c["th"][p] for p in ps])
    ctx = make_ctx(F.fam(c), [c["pts"][p] for p in ps], route)
    rows = []
    ns = [c["pts"][p][1].shape[0] for p in ps]
    tables = {k: [_band_tables(n)[k] for n in ns] for k in _band_tables(130)}
    tables["prior"] = [np.zeros(n, np.int64) for n in ns]
    tables["last"] = [np.where(np.arange(n) == n - 1, n - 1 - 70, -1) for n in ns]
    for name, pfs in tables.items():
        obj, grad, st = ctx.forecast_grad([0, 1], th, pfs)
        assert np.all(st == 0)
        for i, p in enumerate(ps):
            rows.append(_hold(c, p, pfs[i], obj[i], grad[i], f"{route} {name}"))
    none = [np.full(n, -1) for n in ns]
    obj, grad, st = ctx.forecast_grad([0, 1], th, none)
    obj0, _, _ = ctx.forecast_grad([0, 1], th, none, 0)
    ctx.close()
    assert np.all(st == 0) and np.all(obj == 0.0) and np.all(obj0 == 0.0) and np.all(grad == 0.0)
    _assert_held(rows)


def test_upload_order():
    """a grouped upload with the prefix table given in THAT order is held to its own truth (the factor is the grouped one, nothing is
    switched); the time-ordered, interleaved upload of the same observations and the single-output family, where the caller's order
    is the grouped one, are the cases of test_device_within_budget"""
    g = G.case("lmc_sizes")
    p = 5
    m, t, y = g["pts"][p]
    assert np.all(np.diff(m) >= 0) and np.any(np.diff(t) < 0)          # grouped by output, not sorted by time
    c = dict(g, id="lmc_sizes_grouped_upload")
    n = t.shape[0]
    pf = np.where(np.arange(n) % 5 == 0, -1, np.maximum(np.arange(n) - 40, 0))
    ci = F.case("lmc_sizes")
    mi, ti, yi = ci["pts"][p]
    assert np.any(np.diff(mi) < 0)                                      # the interleaved one
    pfi = F.prefix_of(ci, p, 6.0)
    ctx = make_ctx(F.fam(c), [(m, t, y), (mi, ti, yi)])
    th = np.stack([c["th"][p]] * 2)
    obj, grad, st = ctx.forecast_grad([0, 1], th, [pf, pfi])
    ctx.close()
    assert np.all(st == 0)
    _assert_held([_hold(c, p, pf, obj[0], grad[0], "grouped upload"), _hold(ci, p, pfi, obj[1], grad[1], "interleaved upload")])


@pytest.mark.parametrize("route", ROUTES)
def test_objective_is_minus_the_sum_of_forecast_lpd(route):
    """obj (no prior) against medgp_forecast_batch at the same points: within the sum of forecast_ref.lpd_bound over the points plus
    the objective budget; flag_grad = 0 gives the same bits"""
    c = F.case("lmc_sizes")
    P = len(c["pts"])
    th = np.stack(c["th"])
    ctx = make_ctx(F.fam(c), c["pts"], route)
    slots = np.arange(P)
    pfs = [forecast.training_prefix(c["pts"][p][1], 6.0, min_history=1 if p >= 2 else 0) for p in range(P)]
    obj1, grad, st1 = ctx.forecast_grad(slots, th, pfs)
    obj0, none, st0 = ctx.forecast_grad(slots, th, pfs, 0)
    sel = [np.flatnonzero(pf >= 0) for pf in pfs]
    out, st = ctx.forecast(slots, th, [c["pts"][p][0][sel[p]] for p in range(P)], [c["pts"][p][1][sel[p]] for p in range(P)],
                           [pfs[p][sel[p]] for p in range(P)], [c["pts"][p][2][sel[p]] for p in range(P)])
    ctx.close()
    assert none is None and np.all(st0 == 0) and np.all(st1 == 0) and np.all(st == 0)
    assert np.array_equal(obj0.view(np.uint64), obj1.view(np.uint64)), (obj0, obj1)
    for p in range(P):
        lpd = out[p][2]
        tj, _, bj, _ = F.budget_of(c, p, pfs[p])
        bound = FR.lpd_bound() * float(np.sum(np.maximum(1.0, np.abs(lpd)))) + bj * abs(float(tj))
        print(f"FCGRAD-LPD {route} n {c['pts'][p][1].shape[0]}: |obj + sum lpd| {abs(obj1[p] + lpd.sum()):.3g} (bound {bound:.3g})")
        assert abs(obj1[p] + lpd.sum()) <= bound, (p, obj1[p], lpd.sum(), bound)


def _nlml_budget(fam, m, t, y, th):
    """(truth nlml, truth grad, budgets) of medgp_nlml_grad on one patient: nlml_truth's rule on its two numpy fp64 programs"""
    _, tn, tg = T.nlml_grad(*fam, m, t, y, th)
    e = [T.error_pair(*T.nlml_grad(*fam, m, t, y, th, np.float64, variant=v)[1:], tn, tg) for v in ("plain", "device")]
    return tn, tg, T.budget([x[0] for x in e], T.M_NLML), T.budget([x[1] for x in e], T.M_GRAD)


def test_full_history_is_nlml_grad():
    """prefix = NULL at n = 130 (no prior): obj and grad against medgp_nlml_grad of the same patient within the sum of the two
    budgets, each output's error measured against the other call's output on the truth's scale"""
    c = F.case("lmc_sizes")
    p = 5
    m, t, y = c["pts"][p]
    ctx = make_ctx(F.fam(c), [c["pts"][p]])
    th = c["th"][p][None, :]
    obj, grad, st = ctx.forecast_grad([0], th, None)
    nl, gn, stn = ctx.nlml_grad([0], th, True)
    ctx.close()
    assert st[0] == 0 and stn[0] == 0
    tj, tg, bj, bg = F.budget_of(c, p, None)
    tn, tgn, bn, bgn = _nlml_budget(F.fam(c), m, t, y, c["th"][p])
    assert abs(tj - tn) <= 1e-15 * abs(tn)
    ej, eg = T.error_pair(obj[0], grad[0], np.longdouble(nl[0]), gn[0].astype(np.longdouble))
    print(f"FCGRAD-CHAIN n 130: obj {ej:.3g} (bound {bj + bn:.3g}), grad {eg:.3g} (bound {bg + bgn:.3g})")
    assert ej <= bj + bn and eg <= bg + bgn
    _assert_held([_hold(c, p, None, obj[0], grad[0], "full history")])


def test_full_history_is_nlml_grad_at_eight_blocks():
    """n = 512, D = 24, time-sorted (interleaved covariates): no long-double truth.  The bound comes from CPU programs alone: the two
    fp64 programs of the two definitions (forecast_grad_truth.one_factor and nlml_truth.nlml_grad in float64) differ by E; either is
    then off the truth by about E, and each device call gets the budget rule's M x max(E, U64), capped as every budget is."""
    g = G.case("lmc_D24_n512")
    m, t, y = g["pts"][0]
    o = np.argsort(t, kind="stable")
    m, t, y = m[o], t[o], y[o]
    assert np.any(np.diff(m) < 0)
    fam, th = G.fam(g), g["th"][0]
    cj, cg = F.one_factor(*fam, m, t, y, th, None)
    _, nj, ng = T.nlml_grad(*fam, m, t, y, th, np.float64)
    ej, eg = T.error_pair(cj, cg, np.longdouble(nj), ng.astype(np.longdouble))
    bj = 2 * min(F.budget([ej], F.M_OBJ), F.NLML_BUDGET_CAP)
    bg = 2 * min(F.budget([eg], F.M_GRAD), F.GRAD_BUDGET_CAP)
    ctx = make_ctx(fam, [(m, t, y)])
    obj, grad, st = ctx.forecast_grad([0], th[None, :], None)
    nl, gn, stn = ctx.nlml_grad([0], th[None, :], True)
    ctx.close()
    assert st[0] == 0 and stn[0] == 0
    dj, dg = T.error_pair(obj[0], grad[0], np.longdouble(nl[0]), gn[0].astype(np.longdouble))
    print(f"FCGRAD-CHAIN n 512: obj {dj:.3g} (bound {bj:.3g}), grad {dg:.3g} (bound {bg:.3g}); CPU programs apart {ej:.3g}, {eg:.3g}")
    assert dj <= bj and dg <= bg


_CHILD = """
import sys
import numpy as np
import medgp_amd
import forecast_grad_truth as F
c = F.case("lmc_sizes")
ps = [2, 4, 5]
ctx = medgp_amd.Context(*F.fam(c))
ctx.reserve(3, 130, 3)
for s, p in enumerate(ps):
    ctx.set_patient(s, *c["pts"][p])
obj, grad, st = ctx.forecast_grad([0, 1, 2], np.stack([c["th"][p] for p in ps]), [F.prefix_of(c, p, 6.0) for p in ps])
ctx.close()
np.savez(sys.argv[1], obj=obj, grad=grad, st=st)
"""


@pytest.mark.parametrize("fails", [1, 3])
def test_jitter_retries(fails, tmp_path):
    """every quantity is that of the matrix that was factored, K + k diag(sigma^2); the hook is read when the library creates a
    context, in a process of its own"""
    env = dict(os.environ, MEDGP_DEBUG_FAIL_ATTEMPTS=str(fails), PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    out = str(tmp_path / "jitter.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert np.all(z["st"] == fails), z["st"]
    c = F.case("lmc_sizes")
    _assert_held([_hold(c, p, F.prefix_of(c, p, 6.0), z["obj"][i], z["grad"][i], f"jitter{fails}", fails) for i, p in enumerate([2, 4, 5])])


def test_failed_patient_gets_nan_and_spares_its_batch_mates():
    """a patient without noise and with duplicated times fails every retry (as in test_loo_grad_gpu.py)"""
    c = F.case("lmc_sizes")
    D = c["D"]
    sing = (np.zeros(6, np.int32), np.array([1, 1, 1, 2, 2, 2], np.float32), np.ones(6, np.float32))
    pts = [c["pts"][2], sing, c["pts"][4]]
    th = np.stack([c["th"][2], c["th"][3], c["th"][4]])
    th[1, :D] = -80.0
    pfs = [F.prefix_of(c, 2, 6.0), np.arange(6), F.prefix_of(c, 4, 6.0)]
    ctx = make_ctx(F.fam(c), pts, "pinned")
    obj, grad, st = ctx.forecast_grad([0, 1, 2], th, pfs)
    gobj, ggrad, gst = ctx.forecast_grad([0, 2], th[[0, 2]], [pfs[0], pfs[2]])
    obj0, _, st0 = ctx.forecast_grad([0, 1, 2], th, pfs, 0)
    ctx.close()
    assert st[1] == -1 and st0[1] == -1 and st[0] == 0 and st[2] == 0 and np.all(gst == 0), (st, gst)
    assert np.isnan(obj[1]) and np.all(np.isnan(grad[1])) and np.isnan(obj0[1])
    assert np.array_equal(obj[[0, 2]].view(np.uint64), gobj.view(np.uint64))
    assert np.array_equal(np.ascontiguousarray(grad[[0, 2]]).view(np.uint64), ggrad.view(np.uint64))
    _assert_held([_hold(c, p, pfs[i], obj[i], grad[i], "beside a failure") for i, p in ((0, 2), (2, 4))])


def test_priors_enter_as_in_nlml_grad():
    """normal, Laplace and clamp priors on chosen hypers: the objective and every unclamped gradient component move by what they
    move medgp_nlml_grad (the epilogue is shared), to 4 ulps of the largest operand; clamped components are exactly 0"""
    c = F.case("lmc_sizes")
    ps = [2, 3, 5]
    H = c["th"][0].shape[0]
    th = np.stack([c["th"][p] for p in ps])
    pfs = [F.prefix_of(c, p, 6.0) for p in ps]
    ctx = make_ctx(F.fam(c), [c["pts"][p] for p in ps])
    slots = np.arange(3)
    j0, gj0, _ = ctx.forecast_grad(slots, th, pfs)
    n0, gn0, _ = ctx.nlml_grad(slots, th, True)
    flag = np.zeros(H, np.uint8)
    typ = np.full(H, -1, np.int32)
    ex = np.zeros(H, np.uint8)
    p0 = np.zeros(H, np.float32)
    p1 = np.ones(H, np.float32)
    normal, laplace, clamp = [0, 4, 16], [1, 5, 17, 20], [2, 7, 24]
    flag[normal + laplace + clamp] = 1
    typ[normal], typ[laplace], typ[clamp] = 1, 2, 0
    ex[[0, 1, 16, 17, 20]] = 1            # the log-domain hypers among them
    p0[normal + laplace] = [0.3, -0.2, 0.05, 0.25, 0.1, 0.02, 0.5]
    p1[normal + laplace] = [0.5, 2.0, 0.1, 0.7, 1.5, 0.2, 0.9]
    ctx.set_prior(-1, flag, typ, ex, p0, p1)
    j1, gj1, st = ctx.forecast_grad(slots, th, pfs)
    j1o, _, _ = ctx.forecast_grad(slots, th, pfs, 0)
    n1, gn1, _ = ctx.nlml_grad(slots, th, True)
    # nothing scored: the prior term alone
    jn, gjn, _ = ctx.forecast_grad(slots, th, [np.full(pf.shape[0], -1) for pf in pfs])
    ctx.close()
    assert np.all(st == 0)
    assert np.array_equal(j1o.view(np.uint64), j1.view(np.uint64))
    ulp = 2.0 ** -52
    moved = False
    for b in range(3):
        big = max(abs(j0[b]), abs(j1[b]), abs(n0[b]), abs(n1[b]))
        assert abs((j1[b] - j0[b]) - (n1[b] - n0[b])) <= 4 * ulp * big, b
        assert abs(jn[b] - (n1[b] - n0[b])) <= 4 * ulp * big, b
        moved = moved or j1[b] != j0[b]
        for h in range(H):
            if h in clamp:
                assert gj1[b, h] == 0.0 and gn1[b, h] == 0.0 and gjn[b, h] == 0.0
                continue
            big = max(abs(gj0[b, h]), abs(gj1[b, h]), abs(gn0[b, h]), abs(gn1[b, h]))
            assert abs((gj1[b, h] - gj0[b, h]) - (gn1[b, h] - gn0[b, h])) <= 4 * ulp * big, (b, h)
            assert abs(gjn[b, h] - (gn1[b, h] - gn0[b, h])) <= 4 * ulp * big, (b, h)
            if h not in normal + laplace:
                assert gj1[b, h] == gj0[b, h]
    assert moved


def test_bits_do_not_depend_on_the_batch():
    """route pinned: alone, in a batch of 8, the batch reversed"""
    c = F.case("lmc_sizes")
    pts = c["pts"] + [c["pts"][2]]
    th = np.stack(c["th"] + [c["th"][2]])
    pfs = [F.prefix_of(c, p, 6.0) for p in range(7)] + [F.prefix_of(c, 2, 6.0)]
    ctx = make_ctx(F.fam(c), pts, "pinned")
    slots = np.arange(8)
    obj, grad, st = ctx.forecast_grad(slots, th, pfs)
    assert np.all(st == 0)
    robj, rgrad, _ = ctx.forecast_grad(slots[::-1].copy(), th[::-1].copy(), pfs[::-1])
    assert np.array_equal(robj[::-1].view(np.uint64), obj.view(np.uint64))
    assert np.array_equal(np.ascontiguousarray(rgrad[::-1]).view(np.uint64), grad.view(np.uint64))
    for p in range(8):
        o1, g1, _ = ctx.forecast_grad([p], th[p:p + 1], [pfs[p]])
        o0, _, _ = ctx.forecast_grad([p], th[p:p + 1], [pfs[p]], 0)
        assert o1.view(np.uint64)[0] == obj.view(np.uint64)[p] and o0.view(np.uint64)[0] == obj.view(np.uint64)[p], p
        assert np.array_equal(g1[0].view(np.uint64), grad[p].view(np.uint64)), p
    assert np.array_equal(grad[7].view(np.uint64), grad[2].view(np.uint64))
    ctx.close()


def test_other_calls_are_not_disturbed():
    """medgp_posterior_batch, medgp_nlml_grad and medgp_forecast_batch on the same slots return the same bits before and after a
    call; the forecast call selects the very caller-order copies whose batch entries this call pointed elsewhere.  medgp_get_factor
    is refused behind it."""
    c = F.case("lmc_sizes")
    ps = [4, 5, 6]
    pts = [c["pts"][p] for p in ps]
    th = np.stack([c["th"][p] for p in ps])
    pfs = [F.prefix_of(c, p, 6.0) for p in ps]
    ctx = make_ctx(F.fam(c), pts, "pinned")
    slots = np.arange(3)
    ms, ts, ys = [p[0] for p in pts], [p[1] for p in pts], [p[2] for p in pts]

    def others():
        f, _ = ctx.forecast(slots, th, ms, ts, pfs, ys)
        po, _ = ctx.posterior(slots, th, ms, [t + 0.25 for t in ts], parts=False)
        n, g, _ = ctx.nlml_grad(slots, th, True)
        return [x for o in f for x in o] + [x for o in po for x in o[:2]] + [n, g]

    def same(a, b):
        return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))

    before = others()
    obj, grad, st = ctx.forecast_grad(slots, th, pfs)
    with pytest.raises(medgp_amd.MedgpError):
        ctx.get_factor(0, pts[0][1].shape[0])
    f_after, _ = ctx.forecast(slots, th, ms, ts, pfs, ys)            # first: the same effective slots as the call before it
    assert same([x for o in f_after for x in o], before[:9])
    obj2, grad2, _ = ctx.forecast_grad(slots, th, pfs)
    after = others()
    ctx.close()
    assert np.all(st == 0)
    assert same(before, after)
    assert np.array_equal(obj.view(np.uint64), obj2.view(np.uint64)) and np.array_equal(grad.view(np.uint64), grad2.view(np.uint64))


def test_argument_errors():
    c = F.case("lmc_sizes")
    ctx = make_ctx(F.fam(c), c["pts"][1:3])
    th = np.stack(c["th"][1:3])
    n0, n1 = 3, 63
    good = [np.arange(n0), np.arange(n1)]
    for bad in ([np.array([0, 2, 1]), good[1]],                          # above i
                [good[0], np.where(np.arange(n1) == 7, -2, good[1])],      # below -1
                [np.arange(2), good[1]], [good[0], np.arange(n1 + 1)]):    # range lengths
        with pytest.raises(medgp_amd.MedgpError) as e:
            ctx.forecast_grad([0, 1], th, bad)
        assert "error -1" in str(e.value), str(e.value)
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.forecast_grad([0, 1], th, good, 2)
    assert "error -1" in str(e.value) and "flag_grad" in str(e.value)
    slots = np.arange(2, dtype=np.int32)
    obj = np.zeros(2)
    pf = np.concatenate(good).astype(np.int32)
    off = np.array([0, n0, n0 + n1], np.int64)
    i32, dbl = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    call = lambda o, p, g: ctx._lib.medgp_forecast_grad(ctx._h, 2, slots.ctypes.data_as(i32), th.ctypes.data_as(dbl),   # noqa: E731
                                                         o, p, 1, obj.ctypes.data_as(dbl), g, None)
    grad = np.zeros((2, th.shape[1]))
    assert call(off.ctypes.data_as(C.POINTER(C.c_int64)), pf.ctypes.data_as(i32), None) == -1        # NULL grad
    assert call(None, pf.ctypes.data_as(i32), grad.ctypes.data_as(dbl)) == -1                        # prefix without offsets
    assert call(off.ctypes.data_as(C.POINTER(C.c_int64)), pf.ctypes.data_as(i32), grad.ctypes.data_as(dbl)) == 0
    obj2, grad2, st = ctx.forecast_grad([0, 1], th, good)      # the context is still usable
    assert np.all(st == 0) and np.array_equal(obj2.view(np.uint64), obj.view(np.uint64)) and np.array_equal(grad2.view(np.uint64), grad.view(np.uint64))
    ctx.close()
    fam = (7, 17, 3, 2)
    ctx = make_ctx(fam, c["pts"][2:3])
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.forecast_grad([0], synth.theta(1, 0, *fam)[None, :])
    assert "error -1" in str(e.value) and "Q <= 16" in str(e.value)
    ctx.close()
