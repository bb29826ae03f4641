"""medgp_posterior_vjp_batch on the MI355X: the gradient of a loss of the predictions against the long-double truth
(posterior_vjp_truth.py) within the fp64 budget measured on CPU programs alone -- every size at which the kernels take another path,
every edge of the 64-point tile, every family, a covariate with observations and no test point and one with test points and no
observation, on the default routing, the pinned one-workgroup route and the look-ahead route; the built-in losses; the adjoint
identity against medgp_posterior_jvp_batch on the same context; bit invariance (number and position of the cotangent sets, batch,
mean / var, launch chunks, a failed patient beside, the interleaving of the covariates of the points); a jitter retry; NaN outputs;
get_factor; argument and capacity errors; launch counts; predictive.TorchPosterior and jacobian_rows."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
from medgp_amd import predictive
import nlml_truth as T
import posterior_jvp_truth as PJ
import posterior_ref as PR
import posterior_vjp_truth as PV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ["auto", "pinned", "la"]
X = np.longdouble
KINDS = ["nlpd", "sqerr", "crps"]


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


def _points(c, ps):
    pp = [PV.points(c, p) for p in ps]
    return ([x[0] for x in pp] if c["kidx"] == 7 else None), [x[1] for x in pp]


def _cots(c, ps, ncot=PV.NCOT):
    cc = [PV.cotangents(c, p, ncot) for p in ps]
    return [x[0] for x in cc], [x[1] for x in cc]


def _hold(c, p, grad, what, jitter_rounds=0, truth=None):
    """one patient's device gradients ([ncot, H]) against the truth within its budget; prints the observed error.  truth: (grad,
    mag) of other cotangents than the seeded ones (the patient's budget holds for them: the error scale follows the cotangents)"""
    tr, bud = PV.budget_of(c, p, jitter_rounds)
    if truth is not None:
        tr = truth
    if PV.points(c, p)[1].shape[0]:
        assert PV.groups_nonzero(c, tr[0]) and PV.groups_nonzero(c, tr[1]), (what, c["id"], p)      # nothing passes against zeros
    e = PV.error_of(grad, tr[0], tr[1])
    print(f"PVJP-ERR {what} {c['id']}:{p} n {c['pts'][p][1].shape[0]} m {PV.points(c, p)[1].shape[0]}: {e:.3g} (budget {bud:.3g})")
    return (what, c["id"], p, e, bud)


def _assert_held(rows):
    bad = [r for r in rows if not r[3] <= r[4]]
    assert not bad, bad


# every case on the default and the pinned route; the look-ahead leg where the batch holds an entry of more than two 64-blocks
_LEGS = [(s[0], r) for s in PV.LG._SPECS for r in ROUTES if r != "la" or max(n for n, _ in s[5]) > 128]


@pytest.mark.parametrize("cid,route", _LEGS, ids=[f"{c}-{r}" for c, r in _LEGS])
def test_device_within_budget(cid, route, monkeypatch):
    """every case as one (ragged) batch in a shuffled order, two cotangent sets per patient; mean and var within posterior_ref's
    bar, and the gradients the same bits without them"""
    c = PV.case(cid)
    fam = PV.fam(c)
    P = len(c["pts"])
    if route == "la":
        monkeypatch.setenv("MEDGP_MULTI_CU", "1")
    order = np.array([5, 0, 3, 6, 1, 4, 2]) if P == 7 else np.arange(P)
    th = np.stack(c["th"])
    m2l, t2l = _points(c, order)
    cms, cvs = _cots(c, order)
    ctx = make_ctx(fam, c["pts"], route)
    out, st = ctx.posterior_vjp(order, th[order], m2l, t2l, cot_mean=cms, cot_var=cvs)
    out0, st0 = ctx.posterior_vjp(order, th[order], m2l, t2l, cot_mean=cms, cot_var=cvs, want_posterior=False)
    ctx.close()
    assert np.all(st == 0) and np.all(st0 == 0), (st, st0)
    rows = []
    for i, p in enumerate(order):
        mean, var, g = out[i]
        mm = t2l[i].shape[0]
        assert mean.shape == (mm,) and var.shape == (mm,) and g.shape == (PV.NCOT, th.shape[1])
        assert out0[i][0] is None and np.array_equal(_bits(out0[i][2]), _bits(g))          # mean = var = NULL: the same bits
        rows.append(_hold(c, p, g, route))
        if mm:
            m, t, y = c["pts"][p]
            m2 = m2l[i] if m2l is not None else np.zeros(mm, np.int32)
            ref = PR.restate(*fam, m, t, y, th[p], m2, t2l[i])
            PR.check_posterior(fam[0], fam[2], th[p], m2, ref, mean, var)
        else:
            assert not g.any()
    _assert_held(rows)


@pytest.mark.parametrize("kind", KINDS)
def test_builtin_losses(kind):
    """lmc_sizes (n = 1 .. 200, m = 0 .. 130) and the two D = 1 families: the loss against the numpy restatement on the truth's mean
    and var (relative 1e-12 on sum |wt l|), the gradient against the truth of the restatement's cotangents within budget, wt NULL
    against ones bit for bit, a zero weight against the point removed, the fp64 moments against the truth, and the custom kind fed
    the cotangents recomputed in numpy from the device's returned fp64 moments: SQERR bit for bit (its cotangent -2 wt (y - mean) is
    the same two roundings in numpy), NLPD / CRPS within budget (log, division and erf differ in the last bit)."""
    f = predictive.BUILTIN[kind]
    rows = []
    for cid, ps in (("lmc_sizes", list(range(7))), ("sm_Q4", [0]), ("se", [0])):
        c = PV.case(cid)
        fam = PV.fam(c)
        th = np.stack([c["th"][p] for p in ps])
        m2l, t2l = _points(c, ps)
        tg = [PV.targets(c, p) for p in ps]
        y2l, wtl = [x[0] for x in tg], [x[1] for x in tg]
        ones = [np.ones_like(x) for x in y2l]
        ctx = make_ctx(fam, [c["pts"][p] for p in ps], "pinned")
        sl = np.arange(len(ps))
        out, st = ctx.posterior_vjp(sl, th, m2l, t2l, loss=kind, y2_list=y2l, wt_list=wtl, fp64_posterior=True)
        o_none, _ = ctx.posterior_vjp(sl, th, m2l, t2l, loss=kind, y2_list=y2l, want_posterior=False)
        o_ones, _ = ctx.posterior_vjp(sl, th, m2l, t2l, loss=kind, y2_list=y2l, wt_list=ones, want_posterior=False)
        # a zero weight on point 1 of every patient that has two, against the call without that point
        wz = [np.where(np.arange(w.shape[0]) == 1, 0.0, w) for w in wtl]
        keep = [np.arange(w.shape[0]) != 1 for w in wtl]
        o_zero, _ = ctx.posterior_vjp(sl, th, m2l, t2l, loss=kind, y2_list=y2l, wt_list=wz, want_posterior=False)
        o_rem, _ = ctx.posterior_vjp(sl, th, None if m2l is None else [m[k] for m, k in zip(m2l, keep)], [t[k] for t, k in zip(t2l, keep)], loss=kind,
                                     y2_list=[y[k] for y, k in zip(y2l, keep)], wt_list=[w[k] for w, k in zip(wtl, keep)], want_posterior=False)
        cots = [f(o[0], o[1], y, w)[1:] for o, y, w in zip(out, y2l, wtl)]
        o_cus, _ = ctx.posterior_vjp(sl, th, m2l, t2l, cot_mean=[x[0] for x in cots], cot_var=[x[1] for x in cots], want_posterior=False)
        ctx.close()
        assert np.all(st == 0)
        for i, p in enumerate(ps):
            mean64, var64, g, loss = out[i]
            assert np.array_equal(_bits(o_none[i][2]), _bits(o_ones[i][2])) and o_none[i][3] == o_ones[i][3]
            mt, vt = PV.posterior_of(c, p)
            if not mt.shape[0]:
                assert loss == 0.0 and not g.any()
                continue
            val, cm, cv = f(mt, vt, y2l[i].astype(X), wtl[i].astype(X))
            terms = np.array([float(f(mt[j:j + 1], vt[j:j + 1], y2l[i][j:j + 1].astype(X), wtl[i][j:j + 1].astype(X))[0]) for j in range(mt.shape[0])])
            sabs = float(np.sum(np.abs(terms)))
            print(f"PVJP-LOSS {kind} {cid}:{p}: |loss - restatement| / sum|wt l| = {abs(loss - float(val)) / sabs:.3g}")
            assert abs(loss - float(val)) <= 1e-12 * sabs, (cid, p, loss, float(val))
            # the fp64 moments: within the budget of the patient on the scale of their own terms (the JVP truth's forward quantities)
            assert np.max(np.abs(mean64 - mt.astype(np.float64))) <= 1e-9 * max(1.0, float(np.max(np.abs(mt))))
            tr = PV.truth_for(c, p, cm.astype(np.float64), cv.astype(np.float64))
            rows.append(_hold(c, p, g[None, :], kind, truth=tr))
            rows.append(_hold(c, p, o_cus[i][2], kind + "/custom", truth=tr))
            if kind == "sqerr":
                assert np.array_equal(_bits(o_cus[i][2][0]), _bits(g)), (cid, p)
            if mt.shape[0] >= 2:
                _, cmz, cvz = f(mt, vt, y2l[i].astype(X), wz[i].astype(X))
                trz = PV.truth_for(c, p, cmz.astype(np.float64), cvz.astype(np.float64))
                rows.append(_hold(c, p, o_zero[i][2][None, :], kind + "/zero weight", truth=trz))
                rows.append(_hold(c, p, o_rem[i][2][None, :], kind + "/point removed", truth=trz))
    _assert_held(rows)


def test_adjoint_identity_on_the_device():
    """random directions (nvec = 2) and random cotangents on ONE context: grad . v against sum_j cm_j dmean_j(v) + cv_j dvar_j(v) of
    medgp_posterior_jvp_batch.  The bound is the sum of both budgets on their own scales: bud_vjp sum_h scale_h |v_h| for the left
    side, bud_jvp sum_j (|cm_j| scale_mean_j + |cv_j| scale_var_j) for the right."""
    for cid, ps in (("lmc_sizes", [2, 4, 5, 6]), ("lmc_D24_missing", [0]), ("sm_Q4", [0])):
        c = PV.case(cid)
        fam = PV.fam(c)
        th = np.stack([c["th"][p] for p in ps])
        m2l, t2l = _points(c, ps)
        cms, cvs = _cots(c, ps)
        V = np.stack([PJ.directions(c, p, 2) for p in ps])
        ctx = make_ctx(fam, [c["pts"][p] for p in ps])
        sl = np.arange(len(ps))
        og, st = ctx.posterior_vjp(sl, th, m2l, t2l, cot_mean=cms, cot_var=cvs, want_posterior=False)
        oj, st2 = ctx.posterior_jvp(sl, th, m2l, t2l, V, want_posterior=False)
        ctx.close()
        assert np.all(st == 0) and np.all(st2 == 0)
        for i, p in enumerate(ps):
            m, t, y = c["pts"][p]
            (gt, mag), bud_v = PV.budget_of(c, p)
            m2 = m2l[i] if m2l is not None else None
            Pm, alpha = PJ.parts(*fam, m, t, y, th[i], X)
            _, _, gm, gv = PJ.jvp_from_parts(*fam, m, t, th[i], m2, t2l[i], Pm, alpha, V[i], X, True)
            # the JVP budget of THESE points (lmc_D24_missing has its points edited): the JVP truth's rule on its two fp64 programs
            trj = PJ.jvp_from_parts(*fam, m, t, th[i], m2, t2l[i], Pm, alpha, V[i], X, True)
            eg = [PJ.errors(PJ.jvp(*fam, m, t, y, th[i], m2, t2l[i], V[i], np.float64), trj), PJ.errors(PJ.jvp_linalg(*fam, m, t, y, th[i], m2, t2l[i], V[i]), trj)]
            bud_j = min(PJ.budget(eg, PJ.M_PJVP), PJ.GRAD_BUDGET_CAP)
            for k in range(PV.NCOT):
                for d in range(2):
                    lhs = og[i][2][k].astype(X) @ V[i, d].astype(X)
                    rhs = cms[i][:, k].astype(X) @ oj[i][2][:, d].astype(X) + cvs[i][:, k].astype(X) @ oj[i][3][:, d].astype(X)
                    bound = bud_v * float(np.sum(PJ.scale_of(mag[k]) * np.abs(V[i, d]))) + \
                        bud_j * float(np.sum(np.abs(cms[i][:, k]) * PJ.scale_of(gm[:, d]) + np.abs(cvs[i][:, k]) * PJ.scale_of(gv[:, d])))
                    assert bound > 0
                    print(f"PVJP-ADJ {cid}:{p} set {k} dir {d}: {float(abs(lhs - rhs) / bound):.3g} of the bound")
                    assert abs(lhs - rhs) <= bound, (cid, p, k, d)


def test_bits():
    """route pinned: the bits of (entry, set) depend on the patient, theta, its points and that set alone; the points of different
    covariates may be interleaved in any way (the host sorts stably by covariate), the order inside a covariate is part of the input"""
    c = PV.case("lmc_sizes")
    fam = PV.fam(c)
    P = len(c["pts"])
    th = np.stack(c["th"])
    m2l, t2l = _points(c, range(P))
    cm3, cv3 = _cots(c, range(P), 3)
    ctx = make_ctx(fam, c["pts"], "pinned")
    slots = np.arange(P)
    o3, st = ctx.posterior_vjp(slots, th, m2l, t2l, cot_mean=cm3, cot_var=cv3)
    assert np.all(st == 0)

    def same(o, ref, sets=slice(None), what=""):
        for i, (x, r) in enumerate(zip(o, ref)):
            assert np.array_equal(_bits(x[2]), _bits(r[2][sets])), (what, i)

    o1, _ = ctx.posterior_vjp(slots, th, m2l, t2l, cot_mean=[x[:, 1] for x in cm3], cot_var=[x[:, 1] for x in cv3], want_posterior=False)
    assert o1[5][2].shape == (1, th.shape[1])
    same(o1, o3, [1], "ncot 1")
    o2, _ = ctx.posterior_vjp(slots, th, m2l, t2l, cot_mean=[x[:, [2, 0]] for x in cm3], cot_var=[x[:, [2, 0]] for x in cv3], want_posterior=False)
    same(o2, o3, [2, 0], "position")
    rev = slots[::-1].copy()
    orv, _ = ctx.posterior_vjp(rev, th[rev], [m2l[i] for i in rev], [t2l[i] for i in rev], cot_mean=[cm3[i] for i in rev], cot_var=[cv3[i] for i in rev])
    same(orv[::-1], o3, what="batch reversed")
    for x, r in zip(orv[::-1], o3):
        assert np.array_equal(x[0].view(np.uint32), r[0].view(np.uint32)) and np.array_equal(x[1].view(np.uint32), r[1].view(np.uint32))
    for p in (0, 4, 5):
        oa, _ = ctx.posterior_vjp([p], th[p:p + 1], [m2l[p]], [t2l[p]], cot_mean=[cm3[p]], cot_var=[cv3[p]], want_posterior=False)
        same(oa, [o3[p]], what=f"alone {p}")
    # the covariates interleaved another way, the order inside every covariate kept
    g = T._philox(20261605, 0)
    pp = []
    for m2 in m2l:
        keys = g.random(m2.shape[0])
        for d in range(c["D"]):
            keys[m2 == d] = np.sort(keys[m2 == d])
        pp.append(np.argsort(keys, kind="stable"))
    assert any(np.any(q != np.arange(q.shape[0])) for q in pp)
    op, _ = ctx.posterior_vjp(slots, th, [m[q] for m, q in zip(m2l, pp)], [t[q] for t, q in zip(t2l, pp)], cot_mean=[x[q] for x, q in zip(cm3, pp)],
                              cot_var=[x[q] for x, q in zip(cv3, pp)])
    same(op, o3, what="covariates interleaved")
    for x, r, q in zip(op, o3, pp):
        assert np.array_equal(x[0].view(np.uint32), r[0][q].view(np.uint32)) and np.array_equal(x[1].view(np.uint32), r[1][q].view(np.uint32))
    # a failed patient beside (a non-finite theta): NaN in all its outputs, status -1, the batch-mates keep their bits
    thf = th.copy()
    thf[3, 0] = np.nan
    of, stf = ctx.posterior_vjp(slots, thf, m2l, t2l, cot_mean=cm3, cot_var=cv3)
    ob, stb = ctx.posterior_vjp(slots, thf, m2l, t2l, loss="nlpd", y2_list=[PV.targets(c, p)[0] for p in range(P)])
    ctx.close()
    assert stf[3] == -1 and np.all(np.delete(stf, 3) == 0) and stb[3] == -1
    assert np.all(np.isnan(of[3][2])) and np.all(np.isnan(of[3][0])) and np.all(np.isnan(of[3][1]))
    assert np.isnan(ob[3][3]) and np.all(np.isnan(ob[3][2])) and all(np.isfinite(ob[i][3]) and np.all(np.isfinite(ob[i][2])) for i in (0, 1, 2, 4, 5, 6))
    same([of[i] for i in (0, 1, 2, 4, 5, 6)], [o3[i] for i in (0, 1, 2, 4, 5, 6)], what="beside a failure")


_CHILD = """
import sys
import numpy as np
import medgp_amd
import posterior_vjp_truth as PV
mode, path = sys.argv[1], sys.argv[2]
c = PV.case("lmc_sizes")
ps = [2, 3, 5, 6]
ctx = medgp_amd.Context(*PV.fam(c))
ctx.reserve(len(ps), max(c["pts"][p][1].shape[0] for p in ps), len(ps))
for s, p in enumerate(ps):
    ctx.set_patient(s, *c["pts"][p])
if mode != "jitter":
    ctx.pin_route(True)
pp = [PV.points(c, p) for p in ps]
cc = [PV.cotangents(c, p) for p in ps]
args = (np.arange(len(ps)), np.stack([c["th"][p] for p in ps]), [x[0] for x in pp], [x[1] for x in pp])
kw = dict(cot_mean=[x[0] for x in cc], cot_var=[x[1] for x in cc])
res = {}
if mode == "capacity":
    try:
        ctx.posterior_vjp(*args, **kw)
        res["err"] = np.array("")
    except medgp_amd.MedgpError as e:
        res["err"] = np.array(str(e))
    out, st = ctx.posterior(args[0], args[1], args[2], args[3], parts=False)      # the context stays usable
    res["post_st"] = st
else:
    ctx.profile_enable(True)
    ctx.profile_reset()
    out, st = ctx.posterior_vjp(*args, **kw)
    prof = ctx.profile_read()
    res.update(st=st, nsolve=np.array(prof["k_pjvp_solve"][1]), nwgrad=np.array(prof["k_pvjp_wgrad"][1]))
    for i in range(len(ps)):
        res.update({f"mean{i}": out[i][0], f"var{i}": out[i][1], f"g{i}": out[i][2]})
ctx.close()
np.savez(path, **res)
"""
_CHILD_PS = [2, 3, 5, 6]


def _child(mode, tmp_path, **env):
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), **env)
    out = str(tmp_path / f"{mode}.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, mode, out], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


def test_launch_chunks_do_not_change_a_bit(tmp_path):
    """MEDGP_POSTERIOR_BUDGET_GB (read when the context is created, in a process of its own) of 800 KiB: the class of n = 130 (130
    points, three tiles of 256 KiB) and n = 200 (64 points, one tile) is cut between its two entries, the class of n = 63 and 64
    (one tile of 64 KiB each) stays one launch: three k_pjvp_solve launches against two, and every output has the same bits"""
    z = _child("chunks", tmp_path, MEDGP_POSTERIOR_BUDGET_GB=repr(800.0 / 1024 / 1024))
    assert np.all(z["st"] == 0) and int(z["nsolve"]) == 3 and int(z["nwgrad"]) == 3 * PV.NCOT, (z["st"], z["nsolve"], z["nwgrad"])
    c = PV.case("lmc_sizes")
    ps = _CHILD_PS
    m2l, t2l = _points(c, ps)
    cms, cvs = _cots(c, ps)
    ctx = make_ctx(PV.fam(c), [c["pts"][p] for p in ps], "pinned")
    ctx.profile_enable(True)
    ctx.profile_reset()
    out, st = ctx.posterior_vjp(np.arange(4), np.stack([c["th"][p] for p in ps]), m2l, t2l, cot_mean=cms, cot_var=cvs)
    prof = ctx.profile_read()
    ctx.close()
    assert prof["k_pjvp_solve"][1] == 2
    for i in range(4):
        assert np.array_equal(_bits(z[f"g{i}"]), _bits(out[i][2])), i
        assert np.array_equal(z[f"mean{i}"].view(np.uint32), out[i][0].view(np.uint32)) and np.array_equal(z[f"var{i}"].view(np.uint32), out[i][1].view(np.uint32))


def test_jitter_retry(tmp_path):
    """P and alpha are those of the matrix that was factored, K + diag(sigma^2), the derivatives un-jittered; the hook is read when the
    library creates a context, in a process of its own"""
    z = _child("jitter", tmp_path, MEDGP_DEBUG_FAIL_ATTEMPTS="1")
    assert np.all(z["st"] == 1), z["st"]
    c = PV.case("lmc_sizes")
    _assert_held([_hold(c, p, z[f"g{i}"], "jitter1", 1) for i, p in enumerate(_CHILD_PS)])


def test_capacity_error(tmp_path):
    """the 130 points of the n = 130 patient need three tiles of 256 KiB of work rows at once: a budget of 600 KiB refuses the call
    before any device work; the context stays usable"""
    z = _child("capacity", tmp_path, MEDGP_POSTERIOR_BUDGET_GB=repr(600.0 / 1024 / 1024))
    assert np.all(z["post_st"] == 0)
    assert "MEDGP_POSTERIOR_BUDGET_GB" in str(z["err"]) and "-4" in str(z["err"])      # MEDGP_ERR_CAPACITY


def test_nonpositive_variance_is_nan_under_nlpd_and_spares_its_batch_mates():
    """Sixteen SE patients of ONE observation with a noise 1e-9 of the signal and a test point at the observation: K = sf^2 + sigma^2
    rounds to sf^2, so var = (sf^2 - (sf^2 / L)^2) + sigma^2 is a rounding error of either sign plus 1e-18 sf^2.  The entries whose
    returned var is <= 0 have NaN loss and gradient under NLPD and CRPS, finite ones under SQERR; the others are finite and keep the
    bits they have in a call without the bad ones.  Both kinds must occur (asserted), so nothing passes vacuously."""
    fam = (0, 1, 1, 0)
    g = T._philox(20261606, 0)
    P = 16
    pts = [(None, np.array([np.float32(10.0 + s)]), np.array([np.float32(0.5)])) for s in range(P)]
    th = np.stack([np.array([lsf - np.log(1e9), 1.0, lsf]) for lsf in g.uniform(-1.0, 1.0, size=P)])
    t2l = [p[1].copy() for p in pts]
    y2l = [np.array([0.25]) for _ in range(P)]
    ctx = make_ctx(fam, pts, "pinned")
    sl = np.arange(P)
    on, st = ctx.posterior_vjp(sl, th, None, t2l, loss="nlpd", y2_list=y2l)
    oc, _ = ctx.posterior_vjp(sl, th, None, t2l, loss="crps", y2_list=y2l)
    os_, _ = ctx.posterior_vjp(sl, th, None, t2l, loss="sqerr", y2_list=y2l)
    bad = np.array([not o[1][0] > 0 for o in on])
    good = np.flatnonzero(~bad)
    print(f"PVJP-NONPOS var <= 0 in {int(bad.sum())} of {P} entries")
    assert np.all(st == 0) and bad.any() and good.size
    og, _ = ctx.posterior_vjp(good, th[good], None, [t2l[i] for i in good], loss="nlpd", y2_list=[y2l[i] for i in good])
    ctx.close()
    for i in range(P):
        for o in (on, oc):
            assert (np.isnan(o[i][3]) and np.all(np.isnan(o[i][2]))) if bad[i] else (np.isfinite(o[i][3]) and np.all(np.isfinite(o[i][2]))), i
        assert np.isfinite(os_[i][3]) and np.all(np.isfinite(os_[i][2]))
    for j, i in enumerate(good):
        assert np.array_equal(_bits(og[j][2]), _bits(on[i][2])) and og[j][3] == on[i][3]


def test_get_factor_after_the_call_is_that_of_nlml_grad():
    c = PV.case("lmc_sizes")
    p = 5
    n = c["pts"][p][1].shape[0]
    th = c["th"][p][None, :]
    m2l, t2l = _points(c, [p])
    cms, cvs = _cots(c, [p])
    ctx = make_ctx(PV.fam(c), [c["pts"][p]], "pinned")
    ctx.nlml_grad([0], th, False, keep_factor=True)
    a0, l0, b0 = ctx.get_factor(0, n)
    ctx.posterior_vjp([0], th, m2l, t2l, cot_mean=cms, cot_var=cvs)
    a1, l1, b1 = ctx.get_factor(0, n)
    ctx.close()
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)) and np.array_equal(l0.view(np.uint32), l1.view(np.uint32)) and b0 == b1


def test_priors_change_no_bit():
    c = PV.case("lmc_sizes")
    p = 4
    th = c["th"][p][None, :]
    H = th.shape[1]
    m2l, t2l = _points(c, [p])
    cms, cvs = _cots(c, [p])
    ctx = make_ctx(PV.fam(c), [c["pts"][p]], "pinned")
    o0, _ = ctx.posterior_vjp([0], th, m2l, t2l, cot_mean=cms, cot_var=cvs)
    ctx.set_prior(0, np.ones(H, np.uint8), np.ones(H, np.int32), np.zeros(H, np.uint8), np.zeros(H, np.float32), np.ones(H, np.float32))
    o1, _ = ctx.posterior_vjp([0], th, m2l, t2l, cot_mean=cms, cot_var=cvs)
    ctx.close()
    assert np.array_equal(_bits(o0[0][2]), _bits(o1[0][2]))


def test_argument_errors():
    c = PV.case("lmc_sizes")
    ps = [2, 3]
    ctx = make_ctx(PV.fam(c), [c["pts"][p] for p in ps])
    th = np.stack([c["th"][p] for p in ps])
    H = th.shape[1]
    m2l, t2l = _points(c, ps)
    ctx.profile_enable(True)
    ctx.profile_reset()
    slots = np.arange(2, dtype=np.int32)
    off = np.array([0, 63, 127], np.int64)
    m2, t2 = np.concatenate(m2l), np.concatenate(t2l)
    cm, cv, y2 = np.zeros((127, 2)), np.zeros((127, 2)), np.zeros(127)
    grad, loss = np.zeros((2, 2, H)), np.zeros(2)
    i32, dbl, i64, f32 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    ptr = lambda a, ty: a.ctypes.data_as(ty) if a is not None else None

    def call(s=slots, t=th, o=off, kind=0, y=None, w=None, ncot=2, a=cm, b=cv, mean=None, var=None, ls=None, g=grad):
        return ctx._lib.medgp_posterior_vjp_batch(ctx._h, 2, ptr(s, i32), ptr(t, dbl), ptr(o, i64), ptr(m2, i32), ptr(t2, f32), kind, ptr(y, dbl),
                                                  ptr(w, dbl), ncot, ptr(a, dbl), ptr(b, dbl), ptr(mean, f32), ptr(var, f32), ptr(ls, dbl), ptr(g, dbl), None)

    assert call(kind=4) == -1 and call(kind=-1) == -1                                    # an unknown kind
    assert call(ncot=0) == -1
    assert call(kind=1, y=y2, ncot=2, a=None, b=None, ls=loss) == -1                     # ncot != 1 with a built-in kind
    assert call(a=None) == -1 and call(b=None) == -1                                     # missing cotangents
    assert call(y=y2) == -1 and call(ls=loss) == -1 and call(w=y2) == -1                 # superfluous y2 / loss / wt
    assert call(kind=2, y=y2, ncot=1, ls=loss) == -1                                     # superfluous cotangents
    assert call(kind=2, y=None, ncot=1, a=None, b=None, ls=loss) == -1                   # missing y2
    assert call(kind=2, y=y2, ncot=1, a=None, b=None, ls=None) == -1                     # missing loss
    assert call(mean=np.zeros(127, np.float32)) == -1                                    # mean without var
    assert call(s=None) == -1 and call(t=None) == -1 and call(o=None) == -1 and call(g=None) == -1
    assert all(v[1] == 0 for v in ctx.profile_read().values())                           # no device work
    assert call() == 0 and call(kind=3, y=y2, ncot=1, a=None, b=None, ls=loss) == 0      # the context is still usable
    mm = np.zeros(127)
    assert ctx._lib.medgp_posterior_vjp_moments(ctx._h, 126, ptr(mm, dbl), ptr(mm, dbl)) == -1
    ctx.close()
    from medgp_amd import synth
    fam = (7, 17, 3, 2)
    ctx = make_ctx(fam, [c["pts"][2]])
    th17 = synth.theta(1, 0, *fam)[None, :]
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.posterior_vjp([0], th17, [m2l[0]], [t2l[0]], cot_mean=[np.zeros(63)], cot_var=[np.zeros(63)])
    assert "error -1" in str(e.value) and "Q <= 16" in str(e.value)
    ctx.close()


def test_launch_counts():
    """ncot = 2, the seven sizes of lmc_sizes: per size class k_pjvp_solve once (one chunk each at the default budget) and, per
    cotangent set, k_pvjp_cot, k_pvjp_wgrad, k_pvjp_cross and k_pvjp_finish once and two launches under k_epilogue (k_slabsum and
    k_epilogue); nothing per hyper, nothing of the JVP's per-direction kernels"""
    c = PV.case("lmc_sizes")
    P = len(c["pts"])
    m2l, t2l = _points(c, range(P))
    cms, cvs = _cots(c, range(P))
    ctx = make_ctx(PV.fam(c), c["pts"])
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.posterior_vjp(np.arange(P), np.stack(c["th"]), m2l, t2l, cot_mean=cms, cot_var=cvs)
    got = {k: v[1] for k, v in ctx.profile_read().items()}
    cnt, blocks, route = np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros(8, np.int32)
    i32 = C.POINTER(C.c_int32)
    ncls = ctx._lib.medgp_last_plan(ctx._h, 8, cnt.ctypes.data_as(i32), blocks.ctypes.data_as(i32), route.ctypes.data_as(i32))
    ctx.close()
    assert 1 <= ncls <= 4, ncls
    want = dict(k_pjvp_solve=ncls, k_pvjp_cot=2 * ncls, k_pvjp_wgrad=2 * ncls, k_pvjp_cross=2 * ncls, k_pvjp_finish=2 * ncls, k_epilogue=4 * ncls,
                k_fisher_prep=0, k_fisher_kdot=0, k_pjvp_u=0, k_pjvp_dir=0, k_wgrad=0, k_loo_kinv=0, k_posterior=0)
    assert {k: got[k] for k in want} == want, got
    assert ctx._lib.medgp_profile_num_kernels() == 23 and ctx._lib.medgp_profile_num_kernels_all() == 29


def test_torch_posterior_and_jacobian_rows():
    """theta.grad of a torch NLPD equals the built-in NLPD gradient within budget (both form their cotangents from the device's fp64
    mean and var); a smooth custom loss through TorchPosterior equals the custom call fed the same cotangents bit for bit;
    jacobian_rows against the JVP truth's unit directions"""
    import torch
    c = PV.case("lmc_sizes")
    ps = [2, 4]
    fam = PV.fam(c)
    th = np.stack([c["th"][p] for p in ps])
    m2l, t2l = _points(c, ps)
    y2l = [PV.targets(c, p)[0] for p in ps]
    ctx = make_ctx(fam, [c["pts"][p] for p in ps], "pinned")
    y = torch.from_numpy(np.concatenate(y2l))
    tt = torch.tensor(th, dtype=torch.float64, requires_grad=True)
    mean, var = predictive.TorchPosterior.apply(tt, ctx, [0, 1], m2l, t2l)
    assert mean.dtype == torch.float64 and mean.shape == (63 + 65,)
    loss = torch.sum(0.5 * torch.log(2 * np.pi * var) + (y - mean) ** 2 / (2 * var))
    loss.backward()
    ob, _ = ctx.posterior_vjp([0, 1], th, m2l, t2l, loss="nlpd", y2_list=y2l, fp64_posterior=True)
    rows = []
    for i, p in enumerate(ps):
        mt, vt = PV.posterior_of(c, p)
        _, cm, cv = predictive.nlpd(mt, vt, y2l[i].astype(X))
        tr = PV.truth_for(c, p, cm.astype(np.float64), cv.astype(np.float64))
        rows.append(_hold(c, p, tt.grad[i].numpy()[None, :], "torch nlpd", truth=tr))
        rows.append(_hold(c, p, ob[i][2][None, :], "builtin nlpd", truth=tr))
    _assert_held(rows)
    assert abs(float(loss.detach()) - (ob[0][3] + ob[1][3])) <= 1e-12 * abs(float(loss.detach()))
    # a smooth custom loss: sum mean^2 var -- the cotangents torch hands back are 2 mean var and mean^2 of the fp64 moments
    tt2 = torch.tensor(th, dtype=torch.float64, requires_grad=True)
    m_, v_ = predictive.TorchPosterior.apply(tt2, ctx, [0, 1], m2l, t2l)
    torch.sum(m_ * m_ * v_).backward()
    off = [0, 63, 128]
    mm, vv = m_.detach().numpy(), v_.detach().numpy()
    oc, _ = ctx.posterior_vjp([0, 1], th, m2l, t2l, cot_mean=[(2 * mm * vv)[off[i]:off[i + 1]] for i in range(2)],
                              cot_var=[(mm * mm)[off[i]:off[i + 1]] for i in range(2)], want_posterior=False)
    for i in range(2):
        assert np.array_equal(_bits(tt2.grad[i].numpy()), _bits(oc[i][2][0])), i
    # Jacobian rows of two points per patient against the definition
    pts = [np.array([0, 62]), np.array([64, 3])]
    jr, _ = predictive.jacobian_rows(ctx, [0, 1], th, m2l, t2l, pts)
    ctx.close()
    for i, p in enumerate(ps):
        m, t, yy = c["pts"][p]
        assert jr[i][0].shape == (2, th.shape[1])
        cm = np.zeros((t2l[i].shape[0], 4))
        cv = np.zeros((t2l[i].shape[0], 4))
        cm[pts[i], [0, 1]] = 1.0
        cv[pts[i], [2, 3]] = 1.0
        tr = PV.truth_for(c, p, cm, cv)
        d = PV.by_definition(*fam, m, t, yy, th[i], m2l[i], t2l[i], cm, cv)
        assert PV.error_of(d, tr[0], tr[1]) <= 1e-13
        _assert_held([_hold(c, p, np.concatenate([jr[i][0], jr[i][1]]), "jacobian rows", truth=tr)])
