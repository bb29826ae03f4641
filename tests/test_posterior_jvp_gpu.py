"""medgp_posterior_jvp_batch on the MI355X: the directional derivatives of the posterior against the long-double truth
(posterior_jvp_truth.py) within the fp64 budget measured on CPU programs alone, for every size at which the kernels take another path,
every edge of the 64-point tile and every family, on the default routing, the pinned one-workgroup route and the look-ahead route; the
plug-in posterior; the scale identity and linearity; bit invariance (number and position of the directions, batch, order and tile of
the points, upload order, launch chunks); a jitter retry; a failed patient; get_factor; argument and capacity errors;
sensitivity.laplace_predict; launch counts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
from medgp_amd import information, sensitivity
import nlml_truth as T
import posterior_jvp_truth as PT
import posterior_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ["auto", "pinned", "la"]
X = np.longdouble


def make_ctx(fam, pts, route="auto"):
    kidx = fam[0]
    ctx = medgp_amd.Context(*fam)
    ctx.reserve(len(pts), max(max(p[1].shape[0] for p in pts), 1), len(pts))
    for s, (m, t, y) in enumerate(pts):
        ctx.set_patient(s, m if kidx == 7 else None, t, y)
    if route == "pinned":
        ctx.pin_route(True)
    return ctx


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _hold(c, p, dm, dv, what, jitter_rounds=0):
    """one patient's device derivatives (NVEC directions) against the truth within the budget; prints the observed error"""
    tr, bud = PT.budget_of(c, p, jitter_rounds)
    e = PT.errors((dm, dv), tr)
    print(f"PJVP-ERR {what} {c['id']}:{p} n {c['pts'][p][1].shape[0]} m {tr[0].shape[0]}: {e:.3g} (budget {bud:.3g})")
    return (what, c["id"], p, e, bud)


def _assert_held(rows):
    bad = [r for r in rows if not r[3] <= r[4]]
    assert not bad, bad


def _dirs(c, ps, nvec=PT.NVEC):
    return np.stack([PT.directions(c, p, nvec) for p in ps])


def _points(c, ps):
    """(meta2_list or None, t2_list) of the patients ps of a case"""
    pp = [PT.points(c, p) for p in ps]
    return ([x[0] for x in pp] if c["kidx"] == 7 else None), [x[1] for x in pp]


# every case on the default and the pinned route; the look-ahead leg where the batch holds an entry of more than two 64-blocks
_LEGS = [(s[0], r) for s in PT.LG._SPECS for r in ROUTES if r != "la" or max(n for n, _ in s[5]) > 128]


@pytest.mark.parametrize("cid,route", _LEGS, ids=[f"{c}-{r}" for c, r in _LEGS])
def test_device_within_budget(cid, route, monkeypatch):
    """every case as one (ragged) batch in a shuffled order, two directions per patient; mean and var within posterior_ref's bar, and
    the derivative outputs the same bits without them.  la: the look-ahead factorisation forced for the entries that qualify (the knob
    is read when the context is created)"""
    c = PT.case(cid)
    fam = PT.fam(c)
    P = len(c["pts"])
    if route == "la":
        monkeypatch.setenv("MEDGP_MULTI_CU", "1")
    order = np.array([5, 0, 3, 6, 1, 4, 2]) if P == 7 else np.arange(P)
    th = np.stack(c["th"])
    m2l, t2l = _points(c, order)
    ctx = make_ctx(fam, c["pts"], route)
    out, st = ctx.posterior_jvp(order, th[order], m2l, t2l, _dirs(c, order))
    out0, st0 = ctx.posterior_jvp(order, th[order], m2l, t2l, _dirs(c, order), want_posterior=False)
    ctx.close()
    assert np.all(st == 0) and np.all(st0 == 0), (st, st0)
    rows = []
    for i, p in enumerate(order):
        mean, var, dm, dv = out[i]
        mm = t2l[i].shape[0]
        assert mean.shape == (mm,) and var.shape == (mm,) and dm.shape == (mm, PT.NVEC) and dv.shape == (mm, PT.NVEC)
        assert out0[i][0] is None and out0[i][1] is None
        assert np.array_equal(_bits(out0[i][2]), _bits(dm)) and np.array_equal(_bits(out0[i][3]), _bits(dv))      # mean = var = NULL: the same bits
        rows.append(_hold(c, p, dm, dv, route))
        if mm:
            m, t, y = c["pts"][p]
            m2 = m2l[i] if m2l is not None else np.zeros(mm, np.int32)
            ref = PR.restate(*fam, m, t, y, th[p], m2, t2l[i])
            PR.check_posterior(fam[0], fam[2], th[p], m2, ref, mean, var)
    _assert_held(rows)


def test_scale_identity_and_linearity():
    """On the device |dmean . s| <= budget mag and |dvar . s - 2 var_truth| <= budget mag for information.scale_direction s;
    JVP(a u + b v) against a JVP(u) + b JVP(v) within budget (|a| mag_u + |b| mag_v), mag on the scale the budget is defined on
    (posterior_jvp_truth.scale_of)."""
    a, b = 0.75, -1.5
    for cid, ps in (("lmc_sizes", [2, 4, 5, 6]), ("sm_Q4", [0]), ("se", [0])):
        c = PT.case(cid)
        fam = PT.fam(c)
        th = np.stack([c["th"][p] for p in ps])
        V = _dirs(c, ps)
        S = np.stack([information.scale_direction(*fam, t_) for t_ in th])
        Lc = a * V[:, 0] + b * V[:, 1]
        m2l, t2l = _points(c, ps)
        ctx = make_ctx(fam, [c["pts"][p] for p in ps])
        out, st = ctx.posterior_jvp(np.arange(len(ps)), th, m2l, t2l, np.concatenate([V, S[:, None, :], Lc[:, None, :]], axis=1), want_posterior=False)
        ctx.close()
        assert np.all(st == 0)
        for i, p in enumerate(ps):
            m, t, y = c["pts"][p]
            m2 = m2l[i] if m2l is not None else None
            tr, bud = PT.budget_of(c, p)
            _, _, dm, dv = out[i]
            Pm, alpha = PT.parts(*fam, m, t, y, th[i], X)
            _, _, gm, gv = PT.jvp_from_parts(*fam, m, t, th[i], m2, t2l[i], Pm, alpha, S[i], X, True)
            var = PT.posterior_from_parts(*fam, m, t, th[i], m2, t2l[i], Pm, alpha, X)[1]
            em = float(np.max(np.abs(dm[:, 2]) / PT.scale_of(gm[:, 0])))
            ev = float(np.max(np.abs(dv[:, 2].astype(X) - 2 * var) / PT.scale_of(gv[:, 0])))
            print(f"PJVP-SCALE {cid}:{p}: |dmean . s| / mag {em:.3g}, |dvar . s - 2 var| / mag {ev:.3g} (budget {bud:.3g})")
            assert em <= bud and ev <= bud, (p, em, ev, bud)
            for got, k0, mg in ((dm, 0, tr[2]), (dv, 1, tr[3])):
                bound = bud * (abs(a) * PT.scale_of(mg[:, 0]) + abs(b) * PT.scale_of(mg[:, 1]))
                d = np.abs(got[:, 3].astype(X) - (a * got[:, 0].astype(X) + b * got[:, 1].astype(X)))
                print(f"PJVP-LIN {cid}:{p} {'dmean' if k0 == 0 else 'dvar'}: worst {float(np.max(d / bound)):.3g} of the bound")
                assert np.all(d <= bound), (p, k0)


def test_bits():
    """route pinned: the bits of (point, direction) depend on the patient, theta, that point and that direction alone"""
    c = PT.case("lmc_sizes")
    fam = PT.fam(c)
    P = len(c["pts"])
    th = np.stack(c["th"])
    V3 = _dirs(c, range(P), 3)
    m2l, t2l = _points(c, range(P))
    m5, t5, y5 = c["pts"][5]
    # the covariates interleaved at random, every covariate's observations in the order of the grouped upload: the library groups
    # stably, so the patient it works on is the grouped one, row for row
    g = T._philox(20261503, 0)
    keys = g.random(m5.shape[0])
    for d in range(c["D"]):
        keys[m5 == d] = np.sort(keys[m5 == d])
    perm = np.argsort(keys, kind="stable")
    assert np.any(np.diff(m5[perm]) < 0)
    pts = c["pts"] + [(m5[perm], t5[perm], y5[perm])]
    ctx = make_ctx(fam, pts, "pinned")
    slots = np.arange(P)
    o3, st = ctx.posterior_jvp(slots, th, m2l, t2l, V3)
    assert np.all(st == 0)

    def same(o, ref, cols=slice(None), rows=None, what=""):
        for i, (x, r) in enumerate(zip(o, ref)):
            rr = slice(None) if rows is None else rows[i]
            assert np.array_equal(_bits(x[2]), _bits(r[2][rr][:, cols])) and np.array_equal(_bits(x[3]), _bits(r[3][rr][:, cols])), (what, i)

    o1, _ = ctx.posterior_jvp(slots, th, m2l, t2l, V3[:, 1], want_posterior=False)                # nvec = 1 against 3, [nbatch, H] in
    assert o1[5][2].shape == (130, 1)
    same(o1, o3, [1], what="nvec 1")
    o2, _ = ctx.posterior_jvp(slots, th, m2l, t2l, V3[:, [2, 0]], want_posterior=False)           # nvec = 2, every direction at another position
    same(o2, o3, [2, 0], what="position")
    rev = slots[::-1].copy()
    orv, _ = ctx.posterior_jvp(rev, th[rev], [m2l[i] for i in rev], [t2l[i] for i in rev], V3[rev], want_posterior=False)
    same(orv[::-1], o3, what="batch reversed")
    for p in (0, 4, 5):                                                                           # alone
        oa, _ = ctx.posterior_jvp([p], th[p:p + 1], [m2l[p]], [t2l[p]], V3[p:p + 1], want_posterior=False)
        same(oa, [o3[p]], what=f"alone {p}")
    pp = [g.permutation(x.shape[0]) for x in t2l]                                                 # the points permuted
    op, _ = ctx.posterior_jvp(slots, th, [m[q] for m, q in zip(m2l, pp)], [t[q] for t, q in zip(t2l, pp)], V3)
    same(op, o3, rows=pp, what="points permuted")
    for x, r, q in zip(op, o3, pp):
        assert np.array_equal(x[0].view(np.uint32), r[0][q].view(np.uint32)) and np.array_equal(x[1].view(np.uint32), r[1][q].view(np.uint32))
    # a point moved to another tile: the last of patient 4's 65 points (alone in its second tile) against the same point alone
    ol, _ = ctx.posterior_jvp([4], th[4:5], [m2l[4][64:]], [t2l[4][64:]], V3[4:5], want_posterior=False)
    same(ol, [o3[4]], rows=[slice(64, 65)], what="tile")
    ol, _ = ctx.posterior_jvp([5], th[5:6], [m2l[5][[129, 3, 70]]], [t2l[5][[129, 3, 70]]], V3[5:6], want_posterior=False)
    same(ol, [o3[5]], rows=[[129, 3, 70]], what="tile and column")
    ou, stu = ctx.posterior_jvp([P], th[5:6], [m2l[5]], [t2l[5]], V3[5:6], want_posterior=False)  # covariates interleaved on upload
    ctx.close()
    assert np.all(stu == 0)
    same(ou, [o3[5]], what="upload order")


_CHILD = """
import sys
import numpy as np
import medgp_amd
import posterior_jvp_truth as PT
mode, path = sys.argv[1], sys.argv[2]
c = PT.case("lmc_sizes")
ps = [6] if mode == "capacity" else [2, 4, 5]
ctx = medgp_amd.Context(*PT.fam(c))
ctx.reserve(len(ps), max(c["pts"][p][1].shape[0] for p in ps), len(ps))
for s, p in enumerate(ps):
    ctx.set_patient(s, *c["pts"][p])
if mode != "jitter":
    ctx.pin_route(True)
pp = [PT.points(c, p) for p in ps]
args = (np.arange(len(ps)), np.stack([c["th"][p] for p in ps]), [x[0] for x in pp], [x[1] for x in pp], np.stack([PT.directions(c, p) for p in ps]))
res = {}
if mode == "capacity":
    _, _, st = ctx.loo_grad([0], args[1])
    res["loo_st"] = st
    try:
        ctx.posterior_jvp(*args)
        res["err"] = np.array("")
    except medgp_amd.MedgpError as e:
        res["err"] = np.array(str(e))
    out, st = ctx.posterior([0], args[1], args[2], args[3], parts=False)      # the context stays usable
    res["post_st"] = st
else:
    ctx.profile_enable(True)
    ctx.profile_reset()
    out, st = ctx.posterior_jvp(*args)
    prof = ctx.profile_read()
    res.update(st=st, nsolve=np.array(prof["k_pjvp_solve"][1]), ndir=np.array(prof["k_pjvp_dir"][1]))
    for i in range(len(ps)):
        res.update({f"mean{i}": out[i][0], f"var{i}": out[i][1], f"dm{i}": out[i][2], f"dv{i}": out[i][3]})
ctx.close()
np.savez(path, **res)
"""


def _child(mode, tmp_path, **env):
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), **env)
    out = str(tmp_path / f"{mode}.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, mode, out], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


def test_launch_chunks_do_not_change_a_bit(tmp_path):
    """MEDGP_POSTERIOR_BUDGET_GB (read when the context is created, in a process of its own) below one tile's work rows: every tile
    is a launch of its own -- 1 + 2 + 3 tiles for 63, 65 and 130 points -- and every output has the bits of the one-launch call"""
    z = _child("chunks", tmp_path, MEDGP_POSTERIOR_BUDGET_GB="1e-6")
    assert np.all(z["st"] == 0) and int(z["nsolve"]) == 6 and int(z["ndir"]) == 6 * PT.NVEC, (z["st"], z["nsolve"], z["ndir"])
    c = PT.case("lmc_sizes")
    ps = [2, 4, 5]
    m2l, t2l = _points(c, ps)
    ctx = make_ctx(PT.fam(c), [c["pts"][p] for p in ps], "pinned")
    ctx.profile_enable(True)
    ctx.profile_reset()
    out, st = ctx.posterior_jvp(np.arange(3), np.stack([c["th"][p] for p in ps]), m2l, t2l, _dirs(c, ps))
    prof = ctx.profile_read()
    ctx.close()
    assert prof["k_pjvp_solve"][1] < 6
    for i in range(3):
        assert np.array_equal(_bits(z[f"dm{i}"]), _bits(out[i][2])) and np.array_equal(_bits(z[f"dv{i}"]), _bits(out[i][3])), i
        assert np.array_equal(z[f"mean{i}"].view(np.uint32), out[i][0].view(np.uint32)) and np.array_equal(z[f"var{i}"].view(np.uint32), out[i][1].view(np.uint32))


def test_jitter_retry(tmp_path):
    """P and alpha are those of the matrix that was factored, K + diag(sigma^2), the derivatives un-jittered; the hook is read when the
    library creates a context, in a process of its own"""
    z = _child("jitter", tmp_path, MEDGP_DEBUG_FAIL_ATTEMPTS="1")
    assert np.all(z["st"] == 1), z["st"]
    c = PT.case("lmc_sizes")
    _assert_held([_hold(c, p, z[f"dm{i}"], z[f"dv{i}"], "jitter1", 1) for i, p in enumerate([2, 4, 5])])


def test_capacity_error(tmp_path):
    """three 256 x 256 matrices of doubles for the n = 200 patient are 1.5 MiB: a budget of 1.25 MiB holds the two the factorisation
    needs (so medgp_loo_grad runs) and refuses this call; the context stays usable"""
    z = _child("capacity", tmp_path, MEDGP_MEM_BUDGET_GB=repr(1.25 / 1024))
    assert z["loo_st"][0] == 0 and z["post_st"][0] == 0
    assert "MEDGP_MEM_BUDGET_GB" in str(z["err"]) and "-4" in str(z["err"])      # MEDGP_ERR_CAPACITY


def test_failed_patient_gets_nan_and_spares_its_batch_mates():
    """a non-finite theta: NaN in every output of the patient, status -1; its batch-mates keep their bits"""
    c = PT.case("lmc_sizes")
    ps = [2, 3, 4]
    th = np.stack([c["th"][p] for p in ps])
    th[1, 0] = np.nan
    V = _dirs(c, ps)
    m2l, t2l = _points(c, ps)
    ctx = make_ctx(PT.fam(c), [c["pts"][p] for p in ps], "pinned")
    out, st = ctx.posterior_jvp([0, 1, 2], th, m2l, t2l, V)
    o2, st2 = ctx.posterior_jvp([0, 2], th[[0, 2]], [m2l[0], m2l[2]], [t2l[0], t2l[2]], V[[0, 2]])
    ctx.close()
    assert st[1] == -1 and st[0] == 0 and st[2] == 0 and np.all(st2 == 0), (st, st2)
    assert out[1][2].shape == (64, PT.NVEC) and all(np.all(np.isnan(x)) for x in out[1])
    for i, j in ((0, 0), (2, 1)):
        assert np.array_equal(_bits(out[i][2]), _bits(o2[j][2])) and np.array_equal(_bits(out[i][3]), _bits(o2[j][3]))
        assert np.array_equal(out[i][0].view(np.uint32), o2[j][0].view(np.uint32))
    _assert_held([_hold(c, p, out[i][2], out[i][3], "beside a failure") for i, p in ((0, 2), (2, 4))])


def test_get_factor_after_the_call_is_that_of_nlml_grad():
    c = PT.case("lmc_sizes")
    p = 5
    n = c["pts"][p][1].shape[0]
    th = c["th"][p][None, :]
    m2l, t2l = _points(c, [p])
    ctx = make_ctx(PT.fam(c), [c["pts"][p]], "pinned")
    ctx.nlml_grad([0], th, False, keep_factor=True)
    a0, l0, b0 = ctx.get_factor(0, n)
    ctx.posterior_jvp([0], th, m2l, t2l, _dirs(c, [p]))
    a1, l1, b1 = ctx.get_factor(0, n)
    ctx.close()
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)) and np.array_equal(l0.view(np.uint32), l1.view(np.uint32)) and b0 == b1


def test_argument_errors():
    c = PT.case("lmc_sizes")
    ps = [2, 3]
    ctx = make_ctx(PT.fam(c), [c["pts"][p] for p in ps])
    th = np.stack([c["th"][p] for p in ps])
    V = _dirs(c, ps)
    H = th.shape[1]
    m2l, t2l = _points(c, ps)
    ctx.profile_enable(True)
    ctx.profile_reset()
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.posterior_jvp([0, 1], th, m2l, t2l, np.zeros((2, 0, H)))
    assert "error -1" in str(e.value) and "nvec" in str(e.value)
    slots = np.arange(2, dtype=np.int32)
    off = np.array([0, 63, 127], np.int64)
    m2, t2 = np.concatenate(m2l), np.concatenate(t2l)
    dm, dv = np.zeros((127, 2)), np.zeros((127, 2))
    i32, dbl, i64, f32 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    ptr = lambda a, ty: a.ctypes.data_as(ty) if a is not None else None

    def call(s, t, o, nvec, v, a, b):
        return ctx._lib.medgp_posterior_jvp_batch(ctx._h, 2, ptr(s, i32), ptr(t, dbl), ptr(o, i64), ptr(m2, i32), ptr(t2, f32), nvec, ptr(v, dbl),
                                                  None, None, ptr(a, dbl), ptr(b, dbl), None)

    assert call(slots, th, off, 0, V, dm, dv) == -1
    assert call(slots, th, off, -3, V, dm, dv) == -1
    assert call(None, th, off, 2, V, dm, dv) == -1
    assert call(slots, None, off, 2, V, dm, dv) == -1
    assert call(slots, th, None, 2, V, dm, dv) == -1
    assert call(slots, th, off, 2, None, dm, dv) == -1
    assert call(slots, th, off, 2, V, None, dv) == -1
    assert call(slots, th, off, 2, V, dm, None) == -1
    mean = np.zeros(127, np.float32)                                # mean without var
    assert ctx._lib.medgp_posterior_jvp_batch(ctx._h, 2, ptr(slots, i32), ptr(th, dbl), ptr(off, i64), ptr(m2, i32), ptr(t2, f32), 2, ptr(V, dbl),
                                              ptr(mean, f32), None, ptr(dm, dbl), ptr(dv, dbl), None) == -1
    assert all(v[1] == 0 for v in ctx.profile_read().values())      # no device work
    assert call(slots, th, off, 2, V, dm, dv) == 0                  # the context is still usable (mean, var and status NULL)
    ctx.close()
    from medgp_amd import synth
    fam = (7, 17, 3, 2)
    ctx = make_ctx(fam, [c["pts"][2]])
    th17 = synth.theta(1, 0, *fam)[None, :]
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.posterior_jvp([0], th17, [m2l[0]], [t2l[0]], np.ones_like(th17))
    assert "error -1" in str(e.value) and "Q <= 16" in str(e.value)
    ctx.close()


def test_laplace_predict_on_sm_Q4_with_a_rank_3_factor():
    """var_total >= var; var_hyper equals the truth's sum_r dmean_r^2 within the budget: each dmean_r is within budget mag_r of its
    truth, so the sum of squares is within sum_r (2 |dmean_r| + budget mag_r) budget mag_r"""
    c = PT.case("sm_Q4")
    fam = PT.fam(c)
    m, t, y = c["pts"][0]
    th = c["th"][0]
    H = th.shape[0]
    m2, t2 = PT.points(c, 0)
    g = T._philox(20261504, 0)
    B = g.standard_normal((H, H))
    S = sensitivity.covariance_factor(B @ B.T + H * np.eye(H), rank=3)
    assert S.shape == (H, 3)
    ctx = make_ctx(fam, [c["pts"][0]])
    res, st = sensitivity.laplace_predict(ctx, [0], th[None, :], None, [t2], S)
    ctx.close()
    r = res[0]
    assert st[0] == 0 and np.all(r["var_total"] >= r["var"]) and np.all(r["var_hyper"] >= 0)
    assert np.array_equal(r["var_total"], r["var"].astype(np.float64) + r["var_hyper"])
    Pm, alpha = PT.parts(*fam, m, t, y, th, X)
    dm, _, gm, _ = PT.jvp_from_parts(*fam, m, t, th, m2, t2, Pm, alpha, S.T, X, True)
    bud = PT.budget_of(c, 0)[1]
    sc = np.stack([PT.scale_of(gm[:, k]) for k in range(3)], axis=1)
    bound = np.sum((2 * np.abs(dm) + bud * sc) * bud * sc, axis=1)
    err = np.abs(r["var_hyper"].astype(X) - np.sum(dm * dm, axis=1))
    print(f"PJVP-LAPLACE worst {float(np.max(err / bound)):.3g} of the bound; var_hyper / var up to {float(np.max(r['var_hyper'] / r['var'])):.3g}")
    assert np.all(err <= bound)
    PR.assert_fp32_close(r["mean"], PR.restate(*fam, m, t, y, th, np.zeros(t2.shape[0], np.int32), t2)[0], "mean")


def test_launch_counts():
    """nvec = 2, the seven sizes of lmc_sizes: per size class with points k_pjvp_solve once (one chunk each at the default budget) and,
    per direction, k_fisher_prep, k_fisher_kdot, k_pjvp_u and k_pjvp_dir once; nothing of the gradient or Fisher tails"""
    c = PT.case("lmc_sizes")
    P = len(c["pts"])
    m2l, t2l = _points(c, range(P))
    ctx = make_ctx(PT.fam(c), c["pts"])
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.posterior_jvp(np.arange(P), np.stack(c["th"]), m2l, t2l, _dirs(c, range(P)))
    got = {k: v[1] for k, v in ctx.profile_read().items()}
    cnt = np.zeros(8, np.int32)
    blocks = np.zeros(8, np.int32)
    route = np.zeros(8, np.int32)
    i32 = C.POINTER(C.c_int32)
    ncls = ctx._lib.medgp_last_plan(ctx._h, 8, cnt.ctypes.data_as(i32), blocks.ctypes.data_as(i32), route.ctypes.data_as(i32))
    ctx.close()
    assert 1 <= ncls <= 4, ncls
    ns = got["k_pjvp_solve"]
    assert ns == ncls, (ns, ncls)           # every class holds a patient with points: one chunk each
    want = dict(k_pjvp_solve=ns, k_fisher_prep=2 * ns, k_fisher_kdot=2 * ns, k_pjvp_u=2 * ns, k_pjvp_dir=2 * ns, k_fisher_t=0, k_fisher_wgrad=0,
                k_loo_kinv=0, k_wgrad=0, k_epilogue=0, k_alpha=0, k_posterior=0)
    assert {k: got[k] for k in want} == want, got
    assert ctx._lib.medgp_profile_num_kernels() == 23 and ctx._lib.medgp_profile_num_kernels_all() == 29
