"""medgp_set_noise_scale / medgp_hetero_nlml_grad / medgp_hetero_posterior_batch / medgp_robust_nlml_grad on the MI355X against the
long-double truth (hetero_truth.py) within the fp64 budget measured on CPU programs alone: n = 3, 64, 65, an ungrouped caller order
with D = 3, Q = 5, n = 130, SE at n = 64, SM (Q = 3) at n = 100 and Q = 9 at n = 70, on the default, the pinned and the look-ahead
route.  Unit scales are medgp_nlml_grad bit for bit; one forced jitter round re-adds the SCALED noise; the robust call at 0, 1 and 5
sweeps and its warm start; bit invariance; status -1 beside healthy batch-mates; a new patient drops the table; no pointer leaks into
the older calls; argument errors.

Measured on the MI355X (error / budget, worst over the cases and routes): see DESIGN.md section 4.7w."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hetero_truth as HT
import medgp_amd
import nlml_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ["auto", "pinned", "la"]
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


def _eq(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _points(c, ps):
    pp = [HT.points(c, p) for p in ps]
    return ([x[0] for x in pp] if c["kidx"] == 7 else None), [x[1] for x in pp], [x[2] for x in pp]


def _run_all(ctx, c, ps, sl):
    """every output of the four calls for the patients ps in the slots sl of ctx under the case's scales, points and nu:
    {patient index in ps: {output: value}} with the truth's keys, and the status words"""
    th = np.stack([c["th"][p] for p in ps])
    ctx.set_noise_scale(sl, [c["scale"][p] for p in ps])
    r = ctx.hetero_nlml_grad(sl, th)
    m2l, t2l, s2l = _points(c, ps)
    post, pst = ctx.hetero_posterior(sl, th, m2l, t2l, s2l)
    out = [dict(nlml=r["nlml"][i], grad=r["grad"][i], resid=r["resid"][i], fvar=r["fvar"][i], mean=post[i][0], var=post[i][1]) for i in range(len(ps))]
    sts = [r["status"], pst]
    nu = np.stack([c["nu"][p] for p in ps])
    for k in HT.SWEEPS:
        rr = ctx.robust_nlml_grad(sl, th, nu, sweeps=k)
        sts.append(rr["status"])
        for i in range(len(ps)):
            out[i].update({f"r{k}_{o}": (rr[o][i]) for o in HT.ROB_OUTPUTS})
    return out, sts


def _hold(c, p, got, what, jitter_rounds=0):
    """one patient's device outputs against the truth within the budgets; prints error / budget per output"""
    tr, bud = HT.budget_of(c, p, jitter_rounds)
    e = HT.errors(got, tr)
    e.update(HT.post_errors(got, tr["post"]))
    for k in HT.SWEEPS:
        e.update({f"r{k}_{o}": v for o, v in HT.robust_errors({o: got[f"r{k}_{o}"] for o in HT.ROB_OUTPUTS}, tr["rob"][k]).items()})
    assert set(e) == set(bud), set(e) ^ set(bud)
    assert np.any(tr["grad"] != 0) and np.isfinite(float(tr["nlml"]))     # nothing passes against zeros
    rows = []
    for k, v in e.items():
        print(f"HET-ERR {what} {c['id']}:{p} n {c['pts'][p][1].shape[0]} {k}: {v:.3g} / {bud[k]:.3g}")
        rows.append((what, c["id"], p, k, v, bud[k]))
    return rows


def _assert_held(rows):
    bad = [r for r in rows if not r[4] <= r[5]]
    assert not bad, bad


# Every case on the three routes, but for the look-ahead leg of the SE case: its one patient of n = 64 is a single 64-block, which
# k_cholinv<8, 4, 1> factors on every route (the look-ahead schedule takes entries of more than one block) -- the leg would run the
# default leg's kernels again.
_LEGS = [(s[0], r) for s in HT._SPECS for r in ROUTES if r != "la" or max(n for n, _ in s[5]) > 64]


@pytest.mark.parametrize("cid,route", _LEGS, ids=[f"{c}-{r}" for c, r in _LEGS])
def test_unit_scales_are_nlml_grad_bit_for_bit(cid, route, monkeypatch):
    """s = 1 -- no table, and a table of ones -- gives the nlml, gradient and status of medgp_nlml_grad bit for bit: the guard of the
    edit to the assembly"""
    c = HT.case(cid)
    if route == "la":
        monkeypatch.setenv("MEDGP_MULTI_CU", "1")
    P = len(c["pts"])
    sl, th = np.arange(P), np.stack(c["th"])
    ctx = make_ctx(HT.fam(c), c["pts"], route)
    nl, g, st = ctx.nlml_grad(sl, th, True)
    a = ctx.hetero_nlml_grad(sl, th)
    ctx.set_noise_scale(sl, [np.ones(p[1].shape[0]) for p in c["pts"]])
    b = ctx.hetero_nlml_grad(sl, th)
    b0 = ctx.hetero_nlml_grad(sl, th, flag_grad=False, rows=False)
    ctx.close()
    assert np.all(st == 0)
    for r in (a, b):
        assert _eq(r["nlml"], nl) and _eq(r["grad"], g) and np.array_equal(r["status"], st), (cid, route)
    assert _eq(b0["nlml"], nl) and b0["grad"] is None and b0["resid"] is None


@pytest.mark.parametrize("cid,route", _LEGS, ids=[f"{c}-{r}" for c, r in _LEGS])
def test_device_within_budget(cid, route, monkeypatch):
    """every output of all four calls within M_HET max(E_b, E_c, 2^-53) of the truth: random scales in [1/8, 8] on every row (grouped
    rows 0, 63, 64 and the last among them), the batch in a shuffled order; the robust call from ones at 0, 1 and 5 sweeps, and its warm
    start from a returned scale with no sweep reproduces obj and grad bit for bit"""
    c = HT.case(cid)
    if route == "la":
        monkeypatch.setenv("MEDGP_MULTI_CU", "1")
    P = len(c["pts"])
    order = np.roll(np.arange(P), 1)[::-1].copy()
    ctx = make_ctx(HT.fam(c), c["pts"], route)
    out, sts = _run_all(ctx, c, list(order), order)
    th, nu = np.stack([c["th"][p] for p in order]), np.stack([c["nu"][p] for p in order])
    r5 = ctx.robust_nlml_grad(order, th, nu, sweeps=5)
    w0 = ctx.robust_nlml_grad(order, th, nu, sweeps=0, scale0=r5["scale"])
    ctx.close()
    assert all(np.all(s == 0) for s in sts), sts
    assert _eq(w0["obj"], r5["obj"]) and _eq(w0["grad"], r5["grad"]) and np.all(w0["delta"] == 0)
    assert all(_eq(a, b) for a, b in zip(w0["scale"], r5["scale"]))
    rows = []
    for i, p in enumerate(order):
        rows += _hold(c, p, out[i], route)
    _assert_held(rows)


_CHILD_JITTER = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[2])
import hetero_truth as HT
from test_hetero_gpu import make_ctx, _run_all
c = HT.case(HT.JITTER_CASE)
ps = HT.JITTER_PS
ctx = make_ctx(HT.fam(c), [c["pts"][p] for p in ps], sys.argv[3])
out, sts = _run_all(ctx, c, ps, np.arange(len(ps)))
ctx.close()
res = {"sts": np.stack(sts)}
for i in range(len(ps)):
    for k, v in out[i].items():
        res[f"{k}__{i}"] = v
np.savez(sys.argv[1], **res)
"""


@pytest.mark.parametrize("route", ["auto", "la"])
def test_one_jitter_round_adds_the_scaled_noise_again(route, tmp_path):
    """MEDGP_DEBUG_FAIL_ATTEMPTS=1: every quantity is that of the matrix that was factored, K + 2 diag(sigma^2 s); status 1 -- a
    re-assembly that dropped the scales would miss the budget by orders.  The hook is read when the library creates a context, in a
    process of its own"""
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), MEDGP_DEBUG_FAIL_ATTEMPTS="1")
    if route == "la":
        e["MEDGP_MULTI_CU"] = "1"
    out = str(tmp_path / "jit.npz")
    pr = subprocess.run([sys.executable, "-c", _CHILD_JITTER, out, os.path.join(ROOT, "tests"), "auto"], env=e, capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr[-2000:]
    z = np.load(out)
    c = HT.case(HT.JITTER_CASE)
    assert np.all(z["sts"] == 1), z["sts"]
    keys = sorted({k.split("__")[0] for k in z.files if "__" in k})
    rows = []
    for i, p in enumerate(HT.JITTER_PS):
        rows += _hold(c, p, {k: z[f"{k}__{i}"] for k in keys}, "jitter1-" + route, 1)
    _assert_held(rows)


def _row(r, i, keys):
    return [r[k][i] for k in keys if r[k] is not None]


def test_bit_invariance_with_the_route_pinned():
    """an entry's bits depend on its own operands alone: alone, in a batch of 6 or 3, reversed, at another position, at another
    max_batch"""
    c = HT.case("lmc_D3_Q5")
    hk, rk = ("nlml", "grad", "resid", "fvar"), ("obj", "grad", "scale", "delta", "resid", "fvar")
    batch = [3, 1, 2, 3, 0, 1]
    th_of = lambda ps: np.stack([c["th"][p] for p in ps])
    nu_of = lambda ps: np.stack([c["nu"][p] for p in ps])
    full = fullr = None
    for max_batch in (6, 3):
        ctx = make_ctx(HT.fam(c), c["pts"], "pinned", max_batch=max_batch)
        ctx.set_noise_scale(np.arange(4), c["scale"])
        if max_batch == 6:
            full = ctx.hetero_nlml_grad(batch, th_of(batch))
            fullr = ctx.robust_nlml_grad(batch, th_of(batch), nu_of(batch), sweeps=2)
            rev = ctx.hetero_nlml_grad(batch[::-1], th_of(batch[::-1]))
            revr = ctx.robust_nlml_grad(batch[::-1], th_of(batch[::-1]), nu_of(batch[::-1]), sweeps=2)
            for i in range(6):
                assert all(_eq(a, b) for a, b in zip(_row(rev, 5 - i, hk), _row(full, i, hk))), i
                assert all(_eq(a, b) for a, b in zip(_row(revr, 5 - i, rk), _row(fullr, i, rk))), i
            assert all(_eq(a, b) for a, b in zip(_row(full, 0, hk), _row(full, 3, hk)))           # another position
            assert all(_eq(a, b) for a, b in zip(_row(fullr, 1, rk), _row(fullr, 5, rk)))
        for i, p in enumerate(batch[:4]):                                                          # alone, at either max_batch
            one = ctx.hetero_nlml_grad([p], th_of([p]))
            oner = ctx.robust_nlml_grad([p], th_of([p]), nu_of([p]), sweeps=2)
            assert all(_eq(a, b) for a, b in zip(_row(one, 0, hk), _row(full, i, hk))), (max_batch, i)
            assert all(_eq(a, b) for a, b in zip(_row(oner, 0, rk), _row(fullr, i, rk))), (max_batch, i)
        part = ctx.robust_nlml_grad(batch[:3], th_of(batch[:3]), nu_of(batch[:3]), sweeps=2)       # a smaller batch
        assert all(_eq(a, b) for i in range(3) for a, b in zip(_row(part, i, rk), _row(fullr, i, rk))), max_batch
        ctx.close()


def test_status_minus_one_spares_the_batch_mates():
    """an n = 2 entry and an entry whose theta is not finite beside healthy batch-mates: status -1 and NaN rows for them (the n = 2
    entry is served by the posterior call, which has no n > 2 guard), and with the route pinned the batch-mates keep their bits"""
    c = HT.case("lmc_D3_Q5")
    fam = HT.fam(c)
    ps = [1, 2, 3, 1]
    pts = [c["pts"][p] for p in ps]
    m, t, y = c["pts"][1]
    pts.append((m[:2].copy(), t[:2].copy(), y[:2].copy()))              # n = 2
    th = np.stack([c["th"][p] for p in ps] + [c["th"][1]])
    nu = np.stack([c["nu"][p] for p in ps] + [c["nu"][1]])
    scales = [c["scale"][p] for p in ps] + [c["scale"][1][:2]]
    bad = th.copy()
    bad[3, 0] = np.nan
    m2l, t2l, s2l = _points(c, ps + [1])
    ctx = make_ctx(fam, pts, "pinned")
    sl = np.arange(5)
    ctx.set_noise_scale(sl, scales)
    good = ctx.hetero_nlml_grad(sl, th)
    goodr = ctx.robust_nlml_grad(sl, th, nu, sweeps=2)
    gpost, gst = ctx.hetero_posterior(sl, th, m2l, t2l, s2l)
    r = ctx.hetero_nlml_grad(sl, bad)
    rr = ctx.robust_nlml_grad(sl, bad, nu, sweeps=2)
    post, pst = ctx.hetero_posterior(sl, bad, m2l, t2l, s2l)
    ctx.close()
    assert list(good["status"]) == [0, 0, 0, 0, -1] and list(goodr["status"]) == [0, 0, 0, 0, -1] and list(gst) == [0, 0, 0, 0, 0]
    assert list(r["status"]) == [0, 0, 0, -1, -1] and list(rr["status"]) == [0, 0, 0, -1, -1] and list(pst) == [0, 0, 0, -1, 0]
    hk, rk = ("nlml", "grad", "resid", "fvar"), ("obj", "grad", "scale", "delta", "resid", "fvar")
    for i in (3, 4):
        assert all(np.all(np.isnan(v)) for v in _row(r, i, hk)) and all(np.all(np.isnan(v)) for v in _row(rr, i, rk)), i
        assert r["resid"][i].shape == (pts[i][1].shape[0],)
    assert np.all(np.isnan(post[3][0])) and np.all(np.isnan(post[3][1])) and np.all(np.isfinite(gpost[4][0]))
    for i in (0, 1, 2):
        assert all(_eq(a, b) for a, b in zip(_row(r, i, hk), _row(good, i, hk))), i
        assert all(_eq(a, b) for a, b in zip(_row(rr, i, rk), _row(goodr, i, rk))), i
        assert _eq(post[i][0], gpost[i][0]) and _eq(post[i][1], gpost[i][1])


def test_an_entry_that_fails_in_the_middle_of_the_sweeps_ends_at_minus_one():
    """an observation that is not finite: the factorisation of the first sweep succeeds (K does not read y), its E-step leaves scales
    that are not finite and a NaN delta, the next factorisation fails -- status -1 and NaN outputs, decided on the device with no
    read-back between the sweeps; with the route pinned the batch-mates keep the bits they have without it.  An arithmetic outcome,
    not a fault."""
    c = HT.case("lmc_D3_Q5")
    ps = [1, 2]
    m, t, y = c["pts"][1]
    yb = y.copy()
    yb[5] = np.inf
    pts = [c["pts"][p] for p in ps] + [(m, t, yb)]
    th = np.stack([c["th"][p] for p in ps] + [c["th"][1]])
    nu = np.stack([c["nu"][p] for p in ps] + [c["nu"][1]])
    rk = ("obj", "grad", "scale", "delta", "resid", "fvar")
    ctx = make_ctx(HT.fam(c), pts, "pinned")
    for sweeps in (1, 3):
        good = ctx.robust_nlml_grad([0, 1], th[:2], nu[:2], sweeps=sweeps)
        r = ctx.robust_nlml_grad([0, 1, 2], th, nu, sweeps=sweeps)
        assert list(r["status"]) == [0, 0, -1], (sweeps, r["status"])
        assert all(np.all(np.isnan(v)) for v in _row(r, 2, rk)), sweeps
        for i in (0, 1):
            assert all(_eq(a, b) for a, b in zip(_row(r, i, rk), _row(good, i, rk))), (sweeps, i)
    ctx.close()


def test_a_new_patient_drops_the_table_and_no_pointer_leaks():
    """a plain nlml_grad / posterior issued after the heteroscedastic calls is bit-equal to one issued before them; set_patient on a slot
    drops its scales (the call is then medgp_nlml_grad's bits again), the other slots keep theirs; None drops them too"""
    c = HT.case("lmc_D3_Q5")
    P = len(c["pts"])
    sl, th, nu = np.arange(P), np.stack(c["th"]), np.stack(c["nu"])
    m2l, t2l, s2l = _points(c, sl)
    ctx = make_ctx(HT.fam(c), c["pts"], "pinned")
    nl0, g0, st0 = ctx.nlml_grad(sl, th, True)
    p0, _ = ctx.posterior(sl, th, m2l, t2l)
    ctx.set_noise_scale(sl, c["scale"])
    a = ctx.hetero_nlml_grad(sl, th)
    ctx.robust_nlml_grad(sl, th, nu, sweeps=1)
    ctx.hetero_posterior(sl, th, m2l, t2l, s2l)
    nl1, g1, st1 = ctx.nlml_grad(sl, th, True)
    p1, _ = ctx.posterior(sl, th, m2l, t2l)
    assert _eq(nl1, nl0) and _eq(g1, g0) and np.array_equal(st1, st0)
    for i in range(P):
        assert all(np.array_equal(np.asarray(p1[i][j]).view(np.uint32), np.asarray(p0[i][j]).view(np.uint32)) for j in range(2)), i
    assert not _eq(a["nlml"][1:], nl0[1:])                              # the scales did act
    ctx.set_patient(2, *c["pts"][2])
    b = ctx.hetero_nlml_grad(sl, th)
    assert _eq(b["nlml"][2], nl0[2]) and _eq(b["grad"][2], g0[2])
    for i in (0, 1, 3):
        assert _eq(b["nlml"][i], a["nlml"][i]) and _eq(b["grad"][i], a["grad"][i]) and _eq(b["fvar"][i], a["fvar"][i])
    ctx.set_noise_scale([1, 3], None)
    d = ctx.hetero_nlml_grad(sl, th)
    ctx.close()
    assert _eq(d["nlml"][[1, 2, 3]], nl0[[1, 2, 3]]) and _eq(d["nlml"][0], a["nlml"][0])


def test_argument_errors():
    c = HT.case("lmc_D3_Q5")
    ctx = make_ctx(HT.fam(c), c["pts"])
    ps = [1, 2]
    th, nu = np.stack([c["th"][p] for p in ps]), np.stack([c["nu"][p] for p in ps])

    def err(fn):
        with pytest.raises(medgp_amd.MedgpError) as ei:
            fn()
        return str(ei.value)
    for bad in (np.nan, np.inf, 0.0, -1.0, 2.0 ** -41, 2.0 ** 41):
        s = [c["scale"][1].copy(), c["scale"][2].copy()]
        s[1][7] = bad
        msg = err(lambda: ctx.set_noise_scale(ps, s))
        assert "error -1" in msg and "scale[71]" in msg, msg           # 64 rows of the first slot, then row 7
        msg = err(lambda: ctx.robust_nlml_grad(ps, th, nu, scale0=s))
        assert "error -1" in msg and "scale0[71]" in msg, msg
    for bad in (0.0, -2.0, np.nan, np.inf):
        v = nu.copy()
        v[1, 2] = bad
        msg = err(lambda: ctx.robust_nlml_grad(ps, th, v))
        assert "error -1" in msg and "nu[5]" in msg, msg
    assert "error -1" in err(lambda: ctx.robust_nlml_grad(ps, th, nu, sweeps=65))
    assert "error -1" in err(lambda: ctx.robust_nlml_grad(ps, th, nu, sweeps=-1))
    with pytest.raises(ValueError):
        ctx.set_noise_scale(ps, [c["scale"][1], c["scale"][2][:-1]])
    m2l, t2l, s2l = _points(c, ps)
    s2l[0][3] = -1.0
    assert "error -1" in err(lambda: ctx.hetero_posterior(ps, th, m2l, t2l, s2l))
    r = ctx.hetero_nlml_grad(ps, th)                                    # the context stays usable; nothing was made resident
    nl, _, _ = ctx.nlml_grad(ps, th, True)
    assert np.all(r["status"] == 0) and _eq(r["nlml"], nl)
    ctx.close()
    # Q > 16
    from medgp_amd import synth
    g = T._philox(20262121, 0)
    t = np.sort(g.uniform(0, 100, 20)).astype(np.float32)
    ctx = make_ctx((8, 17, 1, 0), [(None, t, g.standard_normal(20).astype(np.float32))])
    th17 = synth.theta(5018, 0, 8, 17, 1, 0)[None]
    assert "error -1" in err(lambda: ctx.hetero_nlml_grad([0], th17))
    assert "error -1" in err(lambda: ctx.robust_nlml_grad([0], th17, 4.0))
    assert "error -1" in err(lambda: ctx.hetero_posterior([0], th17, None, [t[:2]]))
    assert ctx.nlml_grad([0], th17, True)[2][0] == 0
    ctx.close()


def test_profile_entries_of_the_new_kernels():
    """the five kernels are accounted under their own names; the pinned tables keep their lengths"""
    c = HT.case("sm_Q3")
    ctx = make_ctx(HT.fam(c), c["pts"])
    sl, th = np.arange(1), np.stack(c["th"])
    ctx.profile_enable(True, only="k_het_estep")
    ctx.profile_reset()
    ctx.robust_nlml_grad(sl, th, 4.0, sweeps=3)
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    full = ctx.profile_read(all_entries=True)
    ctx.close()
    assert len(prof) == 59 and prof["k_het_estep"][1] == 3 and prof["k_het_estep"][0] > 0 and prof["k_wgrad"][1] == 0
    assert len(full) == 62
