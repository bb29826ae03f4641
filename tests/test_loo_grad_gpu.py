"""medgp_loo_grad on the MI355X: objective and gradient against the long-double truth (loo_grad_truth.py) within the fp64 budget
measured on CPU programs alone, for every size at which the kernels take another path, every family, both factorisation
routes (default routing and the pinned one-workgroup route, as test_loo_gpu.py selects them); agreement with Context.loo; caller
order; bit invariance; jitter retries; a failed patient; priors; argument errors."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
import loo_grad_truth as G
import loo_ref as LR

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


def _hold(c, p, obj, grad, what, jitter_rounds=0):
    """one patient's device output against the truth within the budget; prints the observed errors"""
    tj, tg, bj, bg = G.budget_of(c, p, jitter_rounds)
    ej, eg = G.error_pair(obj, grad, tj, tg)
    print(f"LOOGRAD-ERR {what} {c['id']}:{p} n {c['pts'][p][1].shape[0]}: obj {ej:.3g} (budget {bj:.3g}), grad {eg:.3g} (budget {bg:.3g})")
    return (what, c["id"], p, ej, bj, eg, bg)


def _assert_held(rows):
    bad = [r for r in rows if not (r[3] <= r[4] and r[5] <= r[6])]
    assert not bad, bad


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("cid", G.CASE_IDS)
def test_device_within_budget(cid, route):
    """every patient of the case alone, then (more than one patient) the ragged call mixing all sizes"""
    c = G.case(cid)
    P = len(c["pts"])
    th = np.stack(c["th"])
    ctx = make_ctx(G.fam(c), c["pts"], route)
    rows = []
    for p in range(P):
        obj, grad, st = ctx.loo_grad([p], th[p:p + 1])
        assert st[0] == 0, (p, st)
        rows.append(_hold(c, p, obj[0], grad[0], f"{route} alone"))
    if P > 1:
        order = np.array([5, 0, 3, 6, 1, 4, 2])
        obj, grad, st = ctx.loo_grad(order, th[order])
        assert np.all(st == 0), st
        for i, p in enumerate(order):
            rows.append(_hold(c, p, obj[i], grad[i], f"{route} ragged"))
    ctx.close()
    _assert_held(rows)


@pytest.mark.parametrize("route", ROUTES)
def test_objective_is_minus_the_total_of_loo(route):
    c = G.case("lmc_sizes")
    P = len(c["pts"])
    th = np.stack(c["th"])
    ctx = make_ctx(G.fam(c), c["pts"], route)
    slots = np.arange(P)
    obj1, grad, st1 = ctx.loo_grad(slots, th, True)
    obj0, none, st0 = ctx.loo_grad(slots, th, False)
    out, st, _ = ctx.loo(slots, th, None)
    ctx.close()
    assert none is None and np.all(st0 == 0) and np.all(st1 == 0) and np.all(st == 0)
    assert np.array_equal(obj0.view(np.uint64), obj1.view(np.uint64)), (obj0, obj1)
    for p in range(P):
        tot = out[p][3]
        assert abs(obj1[p] + tot) <= LR.LPD_BOUND * max(1.0, abs(tot)), (p, obj1[p], tot)


def test_caller_order_upload_gives_the_grouped_result():
    c = G.case("lmc_sizes")
    p = 5
    m, t, y = c["pts"][p]
    perm = G.T._philox(20261103, 0).permutation(m.shape[0])
    assert np.any(np.diff(m[perm]) < 0)
    ctx = make_ctx(G.fam(c), [(m, t, y), (m[perm], t[perm], y[perm])])
    th = np.stack([c["th"][p]] * 2)
    obj, grad, st = ctx.loo_grad([0, 1], th)
    ctx.close()
    assert np.all(st == 0)
    _assert_held([_hold(c, p, obj[i], grad[i], f"upload{i}") for i in range(2)])
    _, _, bj, bg = G.budget_of(c, p)
    ej, eg = G.error_pair(obj[1], grad[1], np.longdouble(obj[0]), grad[0].astype(np.longdouble))
    assert ej <= bj and eg <= bg, (ej, bj, eg, bg)


def test_bits_do_not_depend_on_the_batch():
    """route pinned: alone, in a batch of 8, the batch reversed"""
    c = G.case("lmc_sizes")
    pts = c["pts"] + [c["pts"][2]]
    th = np.stack(c["th"] + [c["th"][2]])
    ctx = make_ctx(G.fam(c), pts, "pinned")
    slots = np.arange(8)
    obj, grad, st = ctx.loo_grad(slots, th)
    assert np.all(st == 0)
    robj, rgrad, _ = ctx.loo_grad(slots[::-1].copy(), th[::-1].copy())
    assert np.array_equal(robj[::-1].view(np.uint64), obj.view(np.uint64))
    assert np.array_equal(np.ascontiguousarray(rgrad[::-1]).view(np.uint64), grad.view(np.uint64))
    for p in range(8):
        o1, g1, _ = ctx.loo_grad([p], th[p:p + 1])
        assert o1.view(np.uint64)[0] == obj.view(np.uint64)[p], p
        assert np.array_equal(g1[0].view(np.uint64), grad[p].view(np.uint64)), p
    assert np.array_equal(grad[7].view(np.uint64), grad[2].view(np.uint64))
    ctx.close()


def test_bits_do_not_depend_on_the_batch_from_64_entries_on():
    """route pinned: launches of 64 entries and more deal their tiles XCD-locally (the mapping k_loo_kinv / k_loo_wgrad share with
    k_wgrad).  72 entries, the patients with n = 65, 130, 200 (2, 3, 4 tile rows: off-diagonal tiles, more than two chunks) 24 times
    each; the size classes of a call are launched one by one and n = 65 is a class of its own, so a second call of 72 holds n = 130
    and n = 200 alone, 36 times each: one ragged class of 72.  Every entry has the bits of its patient in a call of 8, through
    medgp_loo_grad and through medgp_nlml_grad."""
    c = G.case("lmc_sizes")
    ps = [4] * 24 + [5] * 36 + [6] * 36                       # the patient of slot s
    th = np.stack([c["th"][p] for p in ps])
    ctx = make_ctx(G.fam(c), [c["pts"][p] for p in ps], "pinned")
    eight = np.array([0, 24, 60, 1, 25, 61, 2, 26])
    mixed = np.stack([np.arange(24), np.arange(24, 48), np.arange(60, 84)], axis=1).ravel()    # 65, 130, 200, 65, ...
    one_class = np.stack([np.arange(24, 60), np.arange(60, 96)], axis=1).ravel()               # 130, 200, 130, ...
    assert mixed.shape[0] == 72 and one_class.shape[0] == 72
    for call in (ctx.loo_grad, lambda s, t: ctx.nlml_grad(s, t, True)):
        obj8, grad8, st8 = call(eight, th[eight])
        assert np.all(st8 == 0), st8
        bits = {ps[s]: (obj8.view(np.uint64)[i], grad8[i].view(np.uint64)) for i, s in list(enumerate(eight))[:3]}
        for slots in (mixed, one_class):
            obj, grad, st = call(slots, th[slots])
            assert np.all(st == 0), st
            for i, s in enumerate(slots):
                assert obj.view(np.uint64)[i] == bits[ps[s]][0], (i, s)
                assert np.array_equal(grad[i].view(np.uint64), bits[ps[s]][1]), (i, s)
    ctx.close()


_CHILD = """
import sys
import numpy as np
import medgp_amd
import loo_grad_truth as G
c = G.case("lmc_sizes")
ps = [2, 4, 5]
ctx = medgp_amd.Context(*G.fam(c))
ctx.reserve(3, 130, 3)
for s, p in enumerate(ps):
    ctx.set_patient(s, *c["pts"][p])
obj, grad, st = ctx.loo_grad([0, 1, 2], np.stack([c["th"][p] for p in ps]))
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
    c = G.case("lmc_sizes")
    _assert_held([_hold(c, p, z["obj"][i], z["grad"][i], f"jitter{fails}", fails) for i, p in enumerate([2, 4, 5])])


def test_failed_patient_gets_nan_and_spares_its_batch_mates():
    """a patient without noise and with duplicated times fails every retry (as in test_loo_gpu.py)"""
    c = G.case("lmc_sizes")
    D = c["D"]
    sing = (np.zeros(6, np.int32), np.array([1, 1, 1, 2, 2, 2], np.float32), np.ones(6, np.float32))
    pts = [c["pts"][2], sing, c["pts"][4]]
    th = np.stack([c["th"][2], c["th"][3], c["th"][4]])
    th[1, :D] = -80.0
    ctx = make_ctx(G.fam(c), pts, "pinned")
    obj, grad, st = ctx.loo_grad([0, 1, 2], th)
    gobj, ggrad, gst = ctx.loo_grad([0, 2], th[[0, 2]])
    obj0, _, st0 = ctx.loo_grad([0, 1, 2], th, False)
    ctx.close()
    assert st[1] == -1 and st0[1] == -1 and st[0] == 0 and st[2] == 0 and np.all(gst == 0), (st, gst)
    assert np.isnan(obj[1]) and np.all(np.isnan(grad[1])) and np.isnan(obj0[1])
    assert np.array_equal(obj[[0, 2]].view(np.uint64), gobj.view(np.uint64))
    assert np.array_equal(np.ascontiguousarray(grad[[0, 2]]).view(np.uint64), ggrad.view(np.uint64))
    _assert_held([_hold(c, p, obj[i], grad[i], "beside a failure") for i, p in ((0, 2), (2, 4))])


def test_priors_enter_as_in_nlml_grad():
    """normal, Laplace and clamp priors on chosen hypers: the objective and every unclamped gradient component move by what they
    move medgp_nlml_grad (the epilogue is shared), to 4 ulps of the largest operand; clamped components are exactly 0"""
    c = G.case("lmc_sizes")
    ps = [2, 3, 5]
    H = c["th"][0].shape[0]
    th = np.stack([c["th"][p] for p in ps])
    ctx = make_ctx(G.fam(c), [c["pts"][p] for p in ps])
    slots = np.arange(3)
    j0, gj0, _ = ctx.loo_grad(slots, th)
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
    j1, gj1, st = ctx.loo_grad(slots, th)
    j1o, _, _ = ctx.loo_grad(slots, th, False)
    n1, gn1, _ = ctx.nlml_grad(slots, th, True)
    ctx.close()
    assert np.all(st == 0)
    assert np.array_equal(j1o.view(np.uint64), j1.view(np.uint64))
    ulp = 2.0 ** -52
    moved = False
    for b in range(3):
        big = max(abs(j0[b]), abs(j1[b]), abs(n0[b]), abs(n1[b]))
        assert abs((j1[b] - j0[b]) - (n1[b] - n0[b])) <= 4 * ulp * big, b
        moved = moved or j1[b] != j0[b]
        for h in range(H):
            if h in clamp:
                assert gj1[b, h] == 0.0 and gn1[b, h] == 0.0
                continue
            big = max(abs(gj0[b, h]), abs(gj1[b, h]), abs(gn0[b, h]), abs(gn1[b, h]))
            assert abs((gj1[b, h] - gj0[b, h]) - (gn1[b, h] - gn0[b, h])) <= 4 * ulp * big, (b, h)
            if h not in normal + laplace:
                assert gj1[b, h] == gj0[b, h]
    assert moved


def test_argument_errors():
    c = G.case("lmc_sizes")
    ctx = make_ctx(G.fam(c), c["pts"][:2])
    th = np.stack(c["th"][:2])
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.loo_grad([0, 1], th, 2)
    assert "error -1" in str(e.value) and "flag_grad" in str(e.value)
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.loo_grad([0, 1], th, 3)
    assert "error -1" in str(e.value)
    slots = np.arange(2, dtype=np.int32)
    obj = np.zeros(2)
    rc = ctx._lib.medgp_loo_grad(ctx._h, 2, slots.ctypes.data_as(C.POINTER(C.c_int32)), th.ctypes.data_as(C.POINTER(C.c_double)), 1,
                                 obj.ctypes.data_as(C.POINTER(C.c_double)), None, None)
    assert rc == -1
    obj, grad, st = ctx.loo_grad([0, 1], th)      # the context is still usable
    assert np.all(st == 0)
    ctx.close()
    from medgp_amd import synth
    fam = (7, 17, 3, 2)
    ctx = make_ctx(fam, c["pts"][2:3])
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.loo_grad([0], synth.theta(1, 0, *fam)[None, :])
    assert "error -1" in str(e.value) and "Q <= 16" in str(e.value)
    ctx.close()
