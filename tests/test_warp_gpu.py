"""medgp_warp_nlml_grad / medgp_warp_posterior_batch on the MI355X against the long-double truth (warp_truth.py) within the fp64 budget
measured on CPU programs alone: every case of warp_truth (n = 3, 17, 63, 64, 65, 130, 200; D = 1 through SE and SM, 3, 24; a kind
that mixes NONE and SAS; covariates without observations; a patient with psi = 0; covariates interleaved; nq = 1, 3, 64) as one ragged
batch on the default, the pinned and the look-ahead route; one jitter round; the identity warps against medgp_nlml_grad; bit
invariance with the route pinned; status -1 beside healthy batch-mates; argument and capacity errors; the ordering of the quantiles;
the older calls' bits around the new calls; and no allocation across repeated evaluations."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
import nlml_truth as T
import warp_truth as WT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ["auto", "pinned", "la"]
X = np.longdouble
OBJ = ("nlml", "grad", "dpsi", "logjac")


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


def _row(r, i):
    return {k: (None if r[k] is None else r[k][i]) for k in OBJ}


def _same(a, b, keys=OBJ):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys if a[k] is not None)


def _same_post(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in WT.POST_OUTPUTS if a[k] is not None)


def _points(c, ps):
    pp = [WT.points(c, p) for p in ps]
    return ([x[0] for x in pp] if c["kidx"] == 7 else None), [x[1] for x in pp], [x[2] for x in pp]


def _post(ctx, c, sl, th, psi, ps):
    m2l, t2l, y2l = _points(c, ps)
    return ctx.warp_posterior(sl, th, psi, m2l, t2l, y2l, kind=c["kind"], zq=c["zq"])


def _hold(c, p, got, what, jitter_rounds=0, post=None):
    """one patient's device outputs against the truth within the budgets; prints error / budget per output"""
    tr, bud = WT.budget_of(c, p, jitter_rounds)
    e = WT.errors(got, tr)
    if post is not None:
        e.update(WT.post_errors(post, tr["post"]))
    assert np.any(tr["grad"] != 0) and np.isfinite(float(tr["nlml"]))     # nothing passes against zeros
    rows = []
    for k, v in e.items():
        print(f"WARP-ERR {what} {c['id']}:{p} n {c['pts'][p][1].shape[0]} {k}: {v:.3g} / {bud[k]:.3g}")
        rows.append((what, c["id"], p, k, v, bud[k]))
    return rows


def _assert_held(rows):
    bad = [r for r in rows if not r[4] <= r[5]]
    assert not bad, bad


_LEGS = [(s[0], r) for s in WT._SPECS for r in ROUTES if r != "la" or max(n for n, _ in s[7]) > 128]


@pytest.mark.parametrize("cid,route", _LEGS, ids=[f"{c}-{r}" for c, r in _LEGS])
def test_device_within_budget(cid, route, monkeypatch):
    """every case as one ragged batch in a shuffled order: nlml, grad, dpsi, logjac and zmean, zvar, quant, lpd within budget;
    flag_grad = 0 gives the same bits of what it returns; dpsi of a covariate without observations or of kind NONE is 0 exactly"""
    c = WT.case(cid)
    P = len(c["pts"])
    if route == "la":
        monkeypatch.setenv("MEDGP_MULTI_CU", "1")
    order = np.roll(np.arange(P), 2)[::-1].copy()
    th, psi = np.stack(c["th"])[order], np.stack(c["psi"])[order]
    ctx = make_ctx(WT.fam(c), c["pts"], route)
    r = ctx.warp_nlml_grad(order, th, psi, kind=c["kind"])
    r0 = ctx.warp_nlml_grad(order, th, psi, kind=c["kind"], flag_grad=False)
    post, pst = _post(ctx, c, order, th, psi, order)
    ctx.close()
    rows = []
    for i, p in enumerate(order):
        tr = WT.truth_of(c, p)
        n = c["pts"][p][1].shape[0]
        if n <= 2 or tr["status"] < 0:
            continue
        assert r["status"][i] == tr["status"] == 0 and pst[i] == 0 and r0["status"][i] == 0, (p, r["status"], pst)
        assert r0["grad"] is None and _same(_row(r0, i), _row(r, i), ("nlml", "dpsi", "logjac"))
        rows += _hold(c, p, _row(r, i), route, post=post[i])
        m = WT._meta(c["kidx"], c["pts"][p][0], n)
        for d in range(WT.nout(c["kidx"], c["D"])):
            if not np.any(m == d) or (c["kind"] is not None and c["kind"][d] == WT.NONE):
                assert not np.any(r["dpsi"][i, d]), (p, d)
        assert np.any(r["dpsi"][i] != 0) and np.any(r["grad"][i] != 0)
    assert len(rows) >= 8 * (P - 1)
    _assert_held(rows)


_CHILD_JITTER = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[2])
import warp_truth as WT
from test_warp_gpu import make_ctx, _post
c = WT.case(WT.JITTER_CASE)
ps = WT.JITTER_PS
th, psi = np.stack([c["th"][p] for p in ps]), np.stack([c["psi"][p] for p in ps])
ctx = make_ctx(WT.fam(c), [c["pts"][p] for p in ps], "pinned")
sl = np.arange(len(ps))
r = ctx.warp_nlml_grad(sl, th, psi, kind=c["kind"])
post, pst = _post(ctx, c, sl, th, psi, ps)
ctx.close()
res = dict(r)
res["pst"] = pst
for i in range(len(ps)):
    for k, v in post[i].items():
        res[f"{k}_{i}"] = v
np.savez(sys.argv[1], **res)
"""


def test_one_jitter_round(tmp_path):
    """every quantity is that of the matrix that was factored, K + diag(sigma^2); status 1.  The hook is read when the library creates
    a context, in a process of its own"""
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), MEDGP_DEBUG_FAIL_ATTEMPTS="1")
    out = str(tmp_path / "jit.npz")
    pr = subprocess.run([sys.executable, "-c", _CHILD_JITTER, out, os.path.join(ROOT, "tests")], env=e, capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr[-2000:]
    z = np.load(out)
    c = WT.case(WT.JITTER_CASE)
    assert np.all(z["status"] == 1) and np.all(z["pst"] == 1), (z["status"], z["pst"])
    rows = []
    for i, p in enumerate(WT.JITTER_PS):
        rows += _hold(c, p, {k: z[k][i] for k in OBJ}, "jitter1", 1, post={k: z[f"{k}_{i}"] for k in WT.POST_OUTPUTS})
    _assert_held(rows)


def test_identity_warps_are_the_plain_nlml_within_the_two_budgets():
    """psi = 0, and kind all NONE, against medgp_nlml_grad of the same context: each within the sum of the two budgets (other summation
    orders: not bits); kind NONE returns dpsi = 0 and logjac = 0 exactly"""
    rows = []
    for cid in ("lmc_D3_Q5", "sm_Q3", "se"):
        c = WT.case(cid)
        fam = WT.fam(c)
        P = len(c["pts"])
        nd = WT.nout(c["kidx"], c["D"])
        th = np.stack(c["th"])
        ctx = make_ctx(fam, c["pts"])
        sl = np.arange(P)
        rz = ctx.warp_nlml_grad(sl, th, np.zeros((nd, 3)))
        rn = ctx.warp_nlml_grad(sl, th, np.stack(c["psi"]), kind=np.zeros(nd, np.int32))
        nl, g, st = ctx.nlml_grad(sl, th, True)
        ctx.close()
        assert not np.any(rn["dpsi"][rn["status"] >= 0]) and not np.any(rn["logjac"][rn["status"] >= 0])
        for p in range(P):
            m, t, y = c["pts"][p]
            if t.shape[0] <= 2:
                assert st[p] == -1 and rz["status"][p] == -1 and rn["status"][p] == -1
                continue
            _, tn, tg = T.nlml_grad(*fam, m, t, y, th[p], X)
            eb = [T.error_pair(*T.float64_program(c, p, 0, v)[1:], tn, tg) for v in ("plain", "device")]
            bn, bg = min(T.budget([x[0] for x in eb], T.M_NLML), T.NLML_BUDGET_CAP), min(T.budget([x[1] for x in eb], T.M_GRAD), T.GRAD_BUDGET_CAP)
            sg = WT.scale_of(tg)
            for what, r, psi, kind in (("psi0", rz, np.zeros((nd, 3)), None), ("none", rn, c["psi"][p], np.zeros(nd, np.int32))):
                pr = WT.programs_for(c, p, psi, kind)
                bud = WT.budgets(pr)
                assert st[p] == 0 and r["status"][p] == 0
                # each call on its own scale: the warp's nlml on nlml_mag, medgp_nlml_grad's on |nlml|; the gradients share theirs
                dn, tol = float(abs(X(r["nlml"][p]) - X(nl[p]))), float(bud["nlml"] * pr["truth"]["nlml_mag"] + bn * abs(tn))
                dg = float(np.max(np.abs(r["grad"][p].astype(X) - g[p].astype(X)) / sg))
                print(f"WARP-ERR {what} {cid}:{p} nlml difference {dn:.3g} / {tol:.3g} grad {dg:.3g} / {bud['grad'] + bg:.3g}")
                rows += [(what, cid, p, "nlml", dn, tol), (what, cid, p, "grad", dg, bud["grad"] + bg)]
    _assert_held(rows)


_CHILD_BITS = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import warp_truth as WT
from test_warp_gpu import make_ctx, _post, _row, _same, _same_post, _points
c = WT.case("lmc_D3_Q5")
psi_of = lambda ps: np.stack([c["psi"][p] for p in ps])
th_of = lambda ps: np.stack([c["th"][p] for p in ps])
batch = [4, 1, 2, 4, 3, 5, 1]
for max_batch in (7, 3):
    ctx = make_ctx(WT.fam(c), c["pts"], "pinned", max_batch=max_batch)
    if max_batch == 7:
        full = ctx.warp_nlml_grad(batch, th_of(batch), psi_of(batch))
        fpost, _ = _post(ctx, c, batch, th_of(batch), psi_of(batch), batch)
        rev = ctx.warp_nlml_grad(batch[::-1], th_of(batch[::-1]), psi_of(batch[::-1]))
        assert _same(_row(full, 0), _row(full, 3)) and _same(_row(full, 1), _row(full, 6))   # another position
        for i, p in enumerate(batch):
            assert _same(_row(rev, 6 - i), _row(full, i)), i
            assert _same_post(fpost[i], fpost[batch.index(p)]), i
    for i, p in enumerate(batch):                                                         # alone, at either max_batch
        one = ctx.warp_nlml_grad([p], th_of([p]), psi_of([p]))
        assert _same(_row(one, 0), _row(full, i)), (max_batch, i)
    part = ctx.warp_nlml_grad(batch[:3], th_of(batch[:3]), psi_of(batch[:3]))            # a smaller batch
    assert all(_same(_row(part, i), _row(full, i)) for i in range(3)), max_batch
    # the points of patient 4 reversed and alone, and a subset of them
    m2l, t2l, y2l = _points(c, [4])
    pr, _ = ctx.warp_posterior([4], th_of([4]), psi_of([4]), [m2l[0][::-1].copy()], [t2l[0][::-1].copy()], [y2l[0][::-1].copy()], zq=c["zq"])
    assert all(np.array_equal(pr[0][k][::-1].view(np.uint64), fpost[0][k].view(np.uint64)) for k in WT.POST_OUTPUTS), max_batch
    ps, _ = ctx.warp_posterior([4], th_of([4]), psi_of([4]), [m2l[0][5:9].copy()], [t2l[0][5:9].copy()], [y2l[0][5:9].copy()], zq=c["zq"])
    assert all(np.array_equal(ps[0][k].view(np.uint64), fpost[0][k][5:9].view(np.uint64)) for k in WT.POST_OUTPUTS), max_batch
    ctx.close()
print("bits ok")
"""


def test_bit_invariance_with_the_route_pinned():
    """an entry's bits depend on its own operands alone: alone, in a batch of 7 or 3, reversed, at another position, at another
    max_batch; a point's not on the other points or their order.  In a process of its own."""
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    pr = subprocess.run([sys.executable, "-c", _CHILD_BITS, os.path.join(ROOT, "tests")], env=e, capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0 and "bits ok" in pr.stdout, pr.stderr[-3000:]


def test_status_minus_one_spares_the_batch_mates():
    """n <= 2 in the objective (not in the posterior), and a lambda at which sinh overflows -- in the fp64 truth too -- on one patient:
    status -1 and NaN outputs, decided on the device; with the route pinned the batch-mates keep their bits.  An arithmetic outcome,
    not a fault."""
    c = WT.case("lmc_D3_Q5")
    fam = WT.fam(c)
    ps = [2, 3, 4, 1]
    pts = [c["pts"][p] for p in ps]
    m, t, y = c["pts"][2]
    pts.append((m[:2].copy(), t[:2].copy(), y[:2].copy()))              # n = 2
    th = np.stack([c["th"][p] for p in ps] + [c["th"][2]])
    psi = np.stack([c["psi"][p] for p in ps] + [c["psi"][2]])
    big = psi.copy()
    big[1, :, 2] = 7.0                                                  # delta = e^7: u = delta asinh(y) - eps beyond sinh's range
    assert WT.objective(*fam, *c["pts"][3], c["th"][3], big[1], None, np.float64)["status"] == -1
    m2l, t2l, y2l = _points(c, ps + [2])
    ctx = make_ctx(fam, pts, "pinned")
    sl = np.arange(5)
    good = ctx.warp_nlml_grad(sl, th, psi)
    gpost, gst = ctx.warp_posterior(sl, th, psi, m2l, t2l, y2l, zq=c["zq"])
    r = ctx.warp_nlml_grad(sl, th, big)
    post, pst = ctx.warp_posterior(sl, th, big, m2l, t2l, y2l, zq=c["zq"])
    again = ctx.warp_nlml_grad(sl, th, psi)
    ctx.close()
    assert list(good["status"]) == [0, 0, 0, 0, -1] and list(gst) == [0, 0, 0, 0, 0]
    assert list(r["status"]) == [0, -1, 0, 0, -1] and list(pst) == [0, -1, 0, 0, 0]
    for i in (1, 4):
        assert all(np.all(np.isnan(r[k][i])) for k in OBJ), i
    assert all(np.all(np.isnan(post[1][k])) for k in WT.POST_OUTPUTS)
    assert all(np.all(np.isfinite(gpost[4][k])) for k in ("zmean", "zvar", "quant"))
    for i in (0, 2, 3):
        assert _same(_row(r, i), _row(good, i)) and _same_post(post[i], gpost[i]), i
    assert all(_same(_row(again, i), _row(good, i)) for i in range(4))


def test_argument_and_capacity_errors(monkeypatch):
    import ctypes as C
    from medgp_amd.capi import _ptr
    c = WT.case("lmc_D3_Q5")
    ctx = make_ctx(WT.fam(c), c["pts"])
    ps = [1, 2]
    th, psi = np.stack([c["th"][p] for p in ps]), np.stack([c["psi"][p] for p in ps])
    m2l, t2l, y2l = _points(c, ps)

    def code(fn):
        with pytest.raises(medgp_amd.MedgpError) as ei:
            fn()
        return int(str(ei.value).split("error ")[1].split(":")[0])
    for bad in (np.nan, np.inf, -np.inf):
        b = psi.copy()
        b[1, 2, 1] = bad
        assert code(lambda: ctx.warp_nlml_grad(ps, th, b)) == -1
        assert code(lambda: ctx.warp_posterior(ps, th, b, m2l, t2l)) == -1
        assert code(lambda: ctx.warp_posterior(ps, th, psi, m2l, t2l, zq=[0.0, bad])) == -1
    for kind in ([1, 2, 1], [-1, 0, 0]):
        assert code(lambda: ctx.warp_nlml_grad(ps, th, psi, kind=kind)) == -1
        assert code(lambda: ctx.warp_posterior(ps, th, psi, m2l, t2l, kind=kind)) == -1
    assert code(lambda: ctx.warp_posterior(ps, th, psi, m2l, t2l, zq=np.zeros(65))) == -1
    # the raw call: nq < 0, the offset and NULL rules
    lib, h = ctx._lib, ctx._h
    sl, st = np.array(ps, np.int32), np.zeros(2, np.int32)
    off = np.array([0, 24, 48], np.int64)
    m2, t2, y2 = np.concatenate(m2l).astype(np.int32), np.concatenate(t2l).astype(np.float32), np.concatenate(y2l).astype(np.float32)
    zq, zm, zv, qu, lp = np.zeros(3), np.zeros(48), np.zeros(48), np.zeros((48, 3)), np.zeros(48)
    i64, i32, f32, f64 = C.c_int64, C.c_int32, C.c_float, C.c_double

    def raw(off=off, m2=m2, t2=t2, y2=y2, nq=3, zq=zq, zm=zm, zv=zv, qu=qu, lp=lp):
        return lib.medgp_warp_posterior_batch(h, 2, _ptr(sl, i32), _ptr(th, f64), None, _ptr(psi, f64), _ptr(off, i64), _ptr(m2, i32), _ptr(t2, f32),
                                              _ptr(y2, f32), nq, _ptr(zq, f64), _ptr(zm, f64), _ptr(zv, f64), _ptr(qu, f64), _ptr(lp, f64), _ptr(st, i32))
    assert raw() == 0 and np.all(st == 0)
    assert raw(nq=-1) == -1 and raw(nq=65) == -1
    assert raw(off=np.array([1, 24, 48], np.int64)) == -1 and raw(off=np.array([0, 30, 24], np.int64)) == -1
    # ... refused before any device work: offsets[0] != 0, offsets that decrease and a covariate outside [0, D) launch and allocate nothing
    ctx.profile_enable(True)
    ctx.profile_reset()
    allocs = ctx.alloc_stats()[1]
    assert raw(off=np.array([1, 24, 48], np.int64)) == -1 and raw(off=np.array([0, 30, 24], np.int64)) == -1 and raw(off=np.array([0, 48, 47], np.int64)) == -1
    bad_m2 = m2.copy()
    bad_m2[47] = 3
    assert raw(m2=bad_m2) == -1 and raw(t2=None) == -1
    assert sum(v[1] for v in ctx.profile_read(all_entries=True).values()) == 0 and ctx.alloc_stats()[1] == allocs
    ctx.profile_enable(False)
    assert raw(off=None) == -1 and raw(t2=None) == -1 and raw(m2=None) == -1
    assert raw(zv=None) == -1 and raw(zm=None) == -1                    # zmean and zvar: both or neither
    assert raw(zq=None) == -1 and raw(nq=0) == -1                       # quant requires nq >= 1 and zq
    assert raw(y2=None) == -1                                           # lpd requires y2
    assert raw(zm=None, zv=None, qu=None, lp=None, y2=None, nq=0, zq=None) == 0   # every output pointer may be NULL
    nl = np.zeros(2)
    assert lib.medgp_warp_nlml_grad(h, 2, _ptr(sl, i32), _ptr(th, f64), None, _ptr(psi, f64), 2, _ptr(nl, f64), None, None, None, None) == -1
    assert lib.medgp_warp_nlml_grad(h, 2, _ptr(sl, i32), _ptr(th, f64), None, None, 1, _ptr(nl, f64), None, None, None, None) == -1
    assert lib.medgp_warp_nlml_grad(h, 2, _ptr(sl, i32), _ptr(th, f64), None, _ptr(psi, f64), 1, None, None, None, None, None) == 0
    r = ctx.warp_nlml_grad(ps, th, psi)                                 # the context stays usable
    assert np.all(r["status"] == 0) and np.all(np.isfinite(r["grad"])) and np.all(np.isfinite(r["dpsi"]))
    ctx.close()
    # Q > 16
    from medgp_amd import synth
    g = T._philox(20261921, 0)
    t = np.sort(g.uniform(0, 100, 20)).astype(np.float32)
    ctx = make_ctx((8, 17, 1, 0), [(None, t, g.standard_normal(20).astype(np.float32))])
    th17 = synth.theta(4918, 0, 8, 17, 1, 0)[None]
    assert code(lambda: ctx.warp_nlml_grad([0], th17, np.zeros((1, 3)))) == -1
    assert code(lambda: ctx.warp_posterior([0], th17, np.zeros((1, 3)), None, [t[:2]])) == -1
    assert ctx.nlml_grad([0], th17, True)[2][0] == 0
    ctx.close()
    # a call beyond one memory wave: the two 256 x 256 matrices of two n = 200 patients are 2 MiB, the budget 1.5 MiB (it is read when
    # the context is created); one of them alone fits
    monkeypatch.setenv("MEDGP_MEM_BUDGET_GB", repr(1.5 / 1024))
    c2 = WT.case("sm_Q3")
    ctx = make_ctx(WT.fam(c2), [c2["pts"][2]] * 2)
    th2, psi2 = np.stack([c2["th"][2]] * 2), np.stack([c2["psi"][2]] * 2)
    assert code(lambda: ctx.warp_nlml_grad([0, 1], th2, psi2)) == -4
    assert code(lambda: ctx.warp_posterior([0, 1], th2, psi2, None, [t[:2]] * 2)) == -4
    one = ctx.warp_nlml_grad([0], th2[:1], psi2[:1])                    # split, the call fits
    ctx.close()
    assert one["status"][0] == 0


def test_quantiles_are_ordered():
    """quant is monotone in zq, and the median lies between the 2.5 % and 97.5 % quantiles (the default probs)"""
    c = WT.case("lmc_D24")
    P = len(c["pts"])
    sl = np.arange(P)
    th, psi = np.stack(c["th"]), np.stack(c["psi"])
    m2l, t2l, _ = _points(c, sl)
    ctx = make_ctx(WT.fam(c), c["pts"])
    q64, st = ctx.warp_posterior(sl, th, psi, m2l, t2l, zq=c["zq"])
    q3, _ = ctx.warp_posterior(sl, th, psi, m2l, t2l)
    ctx.close()
    assert np.all(st == 0)
    for i in range(P):
        assert q64[i]["quant"].shape == (24, 64) and np.all(np.diff(q64[i]["quant"], axis=1) > 0)
        q = q3[i]["quant"]
        assert q.shape == (24, 3) and np.all(q[:, 0] < q[:, 1]) and np.all(q[:, 1] < q[:, 2]) and q3[i]["lpd"] is None
        assert np.array_equal(_bits(q3[i]["zmean"]), _bits(q64[i]["zmean"]))


def test_older_calls_keep_their_bits_around_the_new_calls():
    """nlml_grad, mean_nlml_grad and posterior on the same context return the same bits right before and right after the new calls"""
    c = WT.case("lmc_D3_Q5")
    P = len(c["pts"])
    sl = np.arange(P)
    th, psi = np.stack(c["th"]), np.stack(c["psi"])
    m2l, t2l, y2l = _points(c, sl)
    ctx = make_ctx(WT.fam(c), c["pts"], "pinned")

    def older():
        a = ctx.nlml_grad(sl, th, True)
        b = ctx.mean_nlml_grad(sl, th, np.zeros(3), np.ones(3))
        p, _ = ctx.posterior(sl, th, m2l, t2l)
        return a, b, p
    a0, b0, p0 = older()
    ctx.warp_nlml_grad(sl, th, psi)
    a1, b1, p1 = older()
    ctx.warp_posterior(sl, th, psi, m2l, t2l, y2l, zq=c["zq"])
    a2, b2, p2 = older()
    ctx.close()
    for a, b, p in ((a1, b1, p1), (a2, b2, p2)):
        assert np.array_equal(_bits(a[0]), _bits(a0[0])) and np.array_equal(_bits(a[1]), _bits(a0[1])) and np.array_equal(a[2], a0[2])
        assert all(np.array_equal(_bits(b[k]), _bits(b0[k])) for k in ("nlml", "grad", "dmean", "beta", "beta_cov"))
        for i in range(P):
            for j in range(3):
                assert np.array_equal(np.asarray(p[i][j]).view(np.uint32), np.asarray(p0[i][j]).view(np.uint32)), (i, j)


def test_no_allocation_across_repeated_evaluations():
    """after one warm-up of each call the evaluations obtain no memory: medgp_alloc_stats does not move"""
    c = WT.case("lmc_D3_Q5")
    P = len(c["pts"])
    sl = np.arange(P)
    th, psi = np.stack(c["th"]), np.stack(c["psi"])
    ctx = make_ctx(WT.fam(c), c["pts"], "pinned")
    ctx.warp_nlml_grad(sl, th, psi)
    _post(ctx, c, sl, th, psi, sl)
    before = ctx.alloc_stats()[1:]
    for _ in range(3):
        ctx.warp_nlml_grad(sl, th, psi)
        ctx.warp_nlml_grad(sl, th, psi, flag_grad=False)
        _post(ctx, c, sl, th, psi, sl)
    after = ctx.alloc_stats()[1:]
    ctx.close()
    assert after == before, (before, after)


def test_profile_read_returns_the_warp_kernel_that_was_asked_for():
    """Context.profile_read() keeps the pinned 58-entry table, but a warp kernel named by profile_enable(only=...) is not left out;
    all_entries=True has all 62"""
    c = WT.case("sm_Q3")
    ctx = make_ctx(WT.fam(c), c["pts"])
    sl = np.arange(len(c["pts"]))
    th, psi = np.stack(c["th"]), np.stack(c["psi"])
    ctx.profile_enable(True, only="k_warp_solve")
    ctx.profile_reset()
    ctx.warp_nlml_grad(sl, th, psi)
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    full = ctx.profile_read(all_entries=True)
    plain = ctx.profile_read()
    ctx.close()
    assert len(prof) == 59 and prof["k_warp_solve"][1] >= 1 and prof["k_warp_solve"][0] > 0 and prof["k_wgrad"][1] == 0
    assert len(full) == 62 and len(plain) == 58 and "k_warp_solve" not in plain
