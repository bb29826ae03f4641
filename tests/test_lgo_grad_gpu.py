"""medgp_lgo_grad on the MI355X: objective and gradient against the long-double truth (lgo_grad_truth.py) within the fp64 budget
measured on CPU programs alone -- every 64-block edge under every group scheme, interleaved multi-tile groups, groups of exactly
63 / 64 / 65 members, empty groups, two gradient launches, the single-output families, caller-order upload, one patient of the
headline shape --, both factorisation routes; the identities with Context.loo_grad, Context.nlml_grad and Context.loo; priors;
jitter retries; bit invariance (batch, order, labels, launch chunks); argument errors; a failed patient; get_factor; launch counts."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
from medgp_amd import crossval
import lgo_grad_truth as G
import loo_grad_truth as LG

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


def _hold(c, p, scheme, obj, grad, what, jitter_rounds=0):
    """one patient's device output against the truth within the budget; prints the observed errors"""
    tj, tg, bj, bg = G.budget_of(c, p, scheme, jitter_rounds)
    ej, eg = G.error_pair(obj, grad, tj, tg)
    print(f"LGOGRAD-ERR {what} {c['id']}:{p}:{scheme} n {c['pts'][p][1].shape[0]}: obj {ej:.3g} (budget {bj:.3g}), grad {eg:.3g} (budget {bg:.3g})")
    return (what, c["id"], p, scheme, ej, bj, eg, bg)


def _assert_held(rows):
    bad = [r for r in rows if not (r[4] <= r[5] and r[6] <= r[7])]
    assert not bad, bad


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("scheme", G.SCHEMES)
def test_sizes_under_every_scheme(scheme, route):
    """n = 1, 3, 63, 64, 65 (uploaded in caller order), 130, 200: every patient alone, then the ragged call mixing all sizes"""
    c = G.case("lmc_sizes")
    P = len(c["pts"])
    th = np.stack(c["th"])
    gs = [G.groups_of(c, p, scheme)[0] for p in range(P)]
    ctx = make_ctx(G.fam(c), c["pts"], route)
    rows = []
    for p in range(P):
        obj, grad, st, gst = ctx.lgo_grad([p], th[p:p + 1], [gs[p]])
        assert st[0] == 0 and np.all(gst[0] == 0), (p, st, gst)
        rows.append(_hold(c, p, scheme, obj[0], grad[0], f"{route} alone"))
    order = np.array([5, 0, 3, 6, 1, 4, 2])
    obj, grad, st, gst = ctx.lgo_grad(order, th[order], [gs[p] for p in order])
    assert np.all(st == 0), st
    for i, p in enumerate(order):
        rows.append(_hold(c, p, scheme, obj[i], grad[i], f"{route} ragged"))
    ctx.close()
    _assert_held(rows)


_OTHER = [k for k in G.keys() if not (k[0] == "lmc_sizes" and k[2] in G.SCHEMES)]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("key", _OTHER, ids=[f"{k[0]}-{k[1]}-{k[2]}" for k in _OTHER])
def test_device_within_budget(key, route):
    """interleaved groups of 130 / 65 / 5, groups of 63 / 64 / 65, D = 24 with empty groups, Q = 9, SM, SE, D = 24 n = 512"""
    cid, p, scheme = key
    c = G.case(cid)
    grp, ng = G.groups_of(c, p, scheme)
    if scheme in ("inter", "edges"):
        assert np.any(np.diff(np.flatnonzero(grp == 0)) > 1)          # no contiguous index list
    if cid == "lmc_D24_missing":
        assert np.any(np.bincount(grp, minlength=ng) == 0)            # empty groups
    ctx = make_ctx(G.fam(c), [c["pts"][p]], route)
    obj, grad, st, gst = ctx.lgo_grad([0], c["th"][p][None, :], [grp])
    ctx.close()
    assert st[0] == 0 and np.all(gst[0] == 0)
    _assert_held([_hold(c, p, scheme, obj[0], grad[0], route)])


def test_caller_order_upload_gives_the_grouped_result():
    """the h_perm path: the same patient uploaded grouped and shuffled, the group ids travelling with the observations"""
    c = G.case("lmc_sizes")
    p = 5
    m, t, y = c["pts"][p]
    grp, ng = G.groups_of(c, p, "rand")
    perm = G.T._philox(20261203, 0).permutation(m.shape[0])
    assert np.any(np.diff(m[perm]) < 0)
    ctx = make_ctx(G.fam(c), [(m, t, y), (m[perm], t[perm], y[perm])])
    th = np.stack([c["th"][p]] * 2)
    obj, grad, st, _ = ctx.lgo_grad([0, 1], th, [grp, grp[perm]])
    ctx.close()
    assert np.all(st == 0)
    _assert_held([_hold(c, p, "rand", obj[i], grad[i], f"upload{i}") for i in range(2)])


def test_identities_on_the_device():
    c = G.case("lmc_sizes")
    ps = [2, 4, 5, 6]
    th = np.stack([c["th"][p] for p in ps])
    ctx = make_ctx(G.fam(c), [c["pts"][p] for p in ps])
    slots = np.arange(len(ps))
    ns = [c["pts"][p][1].shape[0] for p in ps]
    # singletons: medgp_loo_grad's quantity, held to ITS truth and budget
    lo, lg, lst = ctx.loo_grad(slots, th)
    so, sg, sst, _ = ctx.lgo_grad(slots, th, [np.arange(n) for n in ns])
    for i, p in enumerate(ps):
        tj, tg, bj, bg = LG.budget_of(c, p)
        for what, o, g in (("loo_grad", lo[i], lg[i]), ("lgo singletons", so[i], sg[i])):
            ej, eg = G.error_pair(o, g, tj, tg)
            print(f"LGOGRAD-ERR {what} {p}: obj {ej:.3g} ({bj:.3g}) grad {eg:.3g} ({bg:.3g})")
            assert ej <= bj and eg <= bg, (what, p, ej, bj, eg, bg)
    # group = NULL: medgp_loo_grad's bits
    no, ngr, nst, ngst = ctx.lgo_grad(slots, th, None)
    assert np.array_equal(_bits(no), _bits(lo)) and np.array_equal(_bits(ngr), _bits(lg)) and np.array_equal(nst, lst)
    assert [g.shape[0] for g in ngst] == ns and all(np.all(g == 0) for g in ngst)
    # one group of everything: the nlml without a prior
    ao, ag, ast, _ = ctx.lgo_grad(slots, th, [np.zeros(n, np.int32) for n in ns])
    mo, mg, mst = ctx.nlml_grad(slots, th, True)
    for i, p in enumerate(ps):
        tj, tg, bj, bg = G.budget_of(c, p, "all")
        for what, o, g in (("lgo one group", ao[i], ag[i]), ("nlml_grad", mo[i], mg[i])):
            ej, eg = G.error_pair(o, g, tj, tg)
            print(f"LGOGRAD-ERR {what} {p}: obj {ej:.3g} ({bj:.3g}) grad {eg:.3g} ({bg:.3g})")
            assert ej <= bj and eg <= bg, (what, p, ej, bj, eg, bg)
    # -total of Context.loo, and the objective-only call
    for scheme in G.SCHEMES:
        gs = [G.groups_of(c, p, scheme)[0] for p in ps]
        o1, g1, st1, _ = ctx.lgo_grad(slots, th, gs)
        o0, g0, st0, _ = ctx.lgo_grad(slots, th, gs, False)
        out, st, _ = ctx.loo(slots, th, gs)
        assert g0 is None and np.all(st0 == 0) and np.all(st1 == 0) and np.all(st == 0)
        assert np.array_equal(_bits(o0), _bits(o1)), (o0, o1)
        for i, p in enumerate(ps):
            bj = G.budget_of(c, p, scheme)[2]
            assert abs(o1[i] + out[i][3]) <= bj * abs(out[i][3]), (scheme, p, o1[i], out[i][3], bj)
    ctx.close()


def test_no_scored_observation_and_hold_out():
    """every id -1: J = 0 and a zero gradient; crossval.hold_out: one group, the rest conditioned on"""
    c = G.case("lmc_sizes")
    p = 4
    n = c["pts"][p][1].shape[0]
    ctx = make_ctx(G.fam(c), [c["pts"][p]])
    obj, grad, st, gst = ctx.lgo_grad([0], c["th"][p][None, :], [np.full(n, -1, np.int32)])
    assert st[0] == 0 and gst[0].shape[0] == 0 and obj[0] == 0.0 and np.all(grad[0] == 0.0)
    grp, ng = G.groups_of(c, p, "hold")
    assert np.array_equal(grp, crossval.hold_out(n, np.arange(10, 30))[0]) and ng == 1
    obj, grad, st, gst = ctx.lgo_grad([0], c["th"][p][None, :], [grp])
    ctx.close()
    assert st[0] == 0 and np.all(gst[0] == 0)
    _assert_held([_hold(c, p, "hold", obj[0], grad[0], "hold_out")])


def test_priors_enter_as_in_nlml_grad():
    """normal, Laplace and clamp priors: obj and grad move by what they move medgp_nlml_grad on the same slot (the epilogue is
    shared): the difference of the two calls is the same with and without the prior, to 1e-12 relative"""
    c = G.case("lmc_sizes")
    ps = [2, 3, 5]
    H = c["th"][0].shape[0]
    th = np.stack([c["th"][p] for p in ps])
    gs = [G.groups_of(c, p, "cov")[0] for p in ps]
    ctx = make_ctx(G.fam(c), [c["pts"][p] for p in ps])
    slots = np.arange(3)
    j0, gj0, _, _ = ctx.lgo_grad(slots, th, gs)
    n0, gn0, _ = ctx.nlml_grad(slots, th, True)
    flag = np.zeros(H, np.uint8)
    typ = np.full(H, -1, np.int32)
    ex = np.zeros(H, np.uint8)
    p0 = np.zeros(H, np.float32)
    p1 = np.ones(H, np.float32)
    normal, laplace, clamp = [0, 4, 16], [1, 5, 17, 20], [2, 7, 24]
    flag[normal + laplace + clamp] = 1
    typ[normal], typ[laplace], typ[clamp] = 1, 2, 0
    ex[[0, 1, 16, 17, 20]] = 1
    p0[normal + laplace] = [0.3, -0.2, 0.05, 0.25, 0.1, 0.02, 0.5]
    p1[normal + laplace] = [0.5, 2.0, 0.1, 0.7, 1.5, 0.2, 0.9]
    ctx.set_prior(-1, flag, typ, ex, p0, p1)
    j1, gj1, st, _ = ctx.lgo_grad(slots, th, gs)
    j1o, _, _, _ = ctx.lgo_grad(slots, th, gs, False)
    n1, gn1, _ = ctx.nlml_grad(slots, th, True)
    ctx.close()
    assert np.all(st == 0)
    assert np.array_equal(_bits(j1o), _bits(j1))
    moved = False
    for b in range(3):
        big = max(abs(j0[b]), abs(j1[b]), abs(n0[b]), abs(n1[b]))
        assert abs((j1[b] - n1[b]) - (j0[b] - n0[b])) <= 1e-12 * big, b
        moved = moved or j1[b] != j0[b]
        for h in range(H):
            if h in clamp:
                assert gj1[b, h] == 0.0 and gn1[b, h] == 0.0
                continue
            big = max(abs(gj0[b, h]), abs(gj1[b, h]), abs(gn0[b, h]), abs(gn1[b, h]))
            assert abs((gj1[b, h] - gn1[b, h]) - (gj0[b, h] - gn0[b, h])) <= 1e-12 * big, (b, h)
    assert moved


@pytest.mark.parametrize("fails", [1, 3])
def test_jitter_retries(fails, monkeypatch):
    """every quantity is that of the matrix that was factored, K + k diag(sigma^2); the hook is read when a context is created"""
    monkeypatch.setenv("MEDGP_DEBUG_FAIL_ATTEMPTS", str(fails))
    c = G.case("lmc_sizes")
    ps = [2, 4, 5]
    gs = [G.groups_of(c, p, "cov")[0] for p in ps]
    ctx = make_ctx(G.fam(c), [c["pts"][p] for p in ps])
    obj, grad, st, gst = ctx.lgo_grad([0, 1, 2], np.stack([c["th"][p] for p in ps]), gs)
    ctx.close()
    assert np.all(st == fails), st
    _assert_held([_hold(c, p, "cov", obj[i], grad[i], f"jitter{fails}", fails) for i, p in enumerate(ps)])


def _relabel(grp, ng, g):
    """the same partition under other labels: a permutation of the ids among ng + 2 (two more unused ones)"""
    perm = g.permutation(ng + 2)
    return np.where(grp >= 0, perm[np.maximum(grp, 0)], -1).astype(np.int32)


@pytest.mark.parametrize("route", ROUTES)
def test_bits(route, monkeypatch):
    """pinned: a patient's bits alone, in a batch of 8, reversed, with relabelled ids and with its groups in >= 2 launch chunks.
    default routing: alone, relabelled and chunked only (the factorisation route may depend on the batch)."""
    c = G.case("lmc_sizes")
    pts = c["pts"] + [c["pts"][6]]
    pp = list(range(7)) + [6]
    th = np.stack(c["th"] + [c["th"][6]])
    gs = [G.groups_of(c, p, "cov")[0] for p in range(6)] + [G.groups_of(c, 6, "inter")[0], G.groups_of(c, 6, "edges")[0]]
    ngs = [3] * 8
    slots = np.arange(8)
    ctx = make_ctx(G.fam(c), pts, route)
    alone = [ctx.lgo_grad([p], th[p:p + 1], [gs[p]]) for p in range(8)]
    if route == "pinned":
        obj, grad, st, _ = ctx.lgo_grad(slots, th, gs)
        assert np.all(st == 0)
        robj, rgrad, _, _ = ctx.lgo_grad(slots[::-1].copy(), th[::-1].copy(), gs[::-1])
        assert np.array_equal(_bits(robj[::-1]), _bits(obj)) and np.array_equal(_bits(rgrad[::-1]), _bits(grad))
        for p in range(8):
            assert _bits(alone[p][0])[0] == _bits(obj)[p] and np.array_equal(_bits(alone[p][1][0]), _bits(grad[p])), p
    g = G.T._philox(20261204, 0)
    for p in range(8):
        o, gr, st, gst = ctx.lgo_grad([p], th[p:p + 1], [_relabel(gs[p], ngs[p], g)])
        assert np.array_equal(_bits(o), _bits(alone[p][0])) and np.array_equal(_bits(gr), _bits(alone[p][1])), ("relabelled", p)
    ctx.close()
    # a block of up to 64 members takes 66.5 kB, of 65 .. 128 264 kB, of 129 .. 192 593 kB.  Budgets (1 GB = 2^30 bytes) under which the
    # groups of the patient no longer share a launch chunk: three blocks of 66.5 kB under 107 kB; 593 | 264 + 66.5 under 644 kB;
    # 66.5 + 66.5 | 264 under 322 kB
    for p, gb in ((5, "1e-4"), (6, "6e-4"), (7, "3e-4")):
        assert p != 5 or np.bincount(gs[5]).max() <= 64
        monkeypatch.setenv("MEDGP_POSTERIOR_BUDGET_GB", gb)
        ctx = make_ctx(G.fam(c), pts[p:p + 1], route)
        ctx.profile_enable(True)
        o, gr, st, gst = ctx.lgo_grad([0], th[p:p + 1], [gs[p]])
        prof = ctx.profile_read()
        ctx.close()
        assert prof["k_lgo_s"][1] >= 2 and prof["k_lgo_s"][1] == prof["k_lgo_t"][1] == prof["k_loo_gram"][1], (p, prof)
        assert np.array_equal(_bits(o), _bits(alone[p][0])) and np.array_equal(_bits(gr), _bits(alone[p][1])), ("chunked", p)


def test_single_group_beyond_the_budget_is_a_capacity_error(monkeypatch):
    monkeypatch.setenv("MEDGP_POSTERIOR_BUDGET_GB", "1e-5")
    c = G.case("lmc_sizes")
    ctx = make_ctx(G.fam(c), [c["pts"][5]])
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.lgo_grad([0], c["th"][5][None, :], [G.groups_of(c, 5, "cov")[0]])
    assert "MEDGP_POSTERIOR_BUDGET_GB" in str(e.value) and "-4" in str(e.value)   # MEDGP_ERR_CAPACITY
    ctx.close()


def test_argument_errors():
    c = G.case("lmc_sizes")
    ctx = make_ctx(G.fam(c), c["pts"][2:4])
    th = np.stack(c["th"][2:4])
    gs = [G.groups_of(c, p, "cov")[0] for p in (2, 3)]
    ctx.profile_enable(True)
    ctx.profile_reset()
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.lgo_grad([0, 1], th, gs, 2)
    assert "error -1" in str(e.value) and "flag_grad" in str(e.value)
    slots = np.arange(2, dtype=np.int32)
    obj, grad = np.zeros(2), np.zeros((2, ctx.H))
    grp = np.concatenate(gs).astype(np.int32)
    ng = np.array([3, 3], np.int32)
    i32, dbl = C.POINTER(C.c_int32), C.POINTER(C.c_double)

    def call(grp_, ng_, flag, grad_):
        return ctx._lib.medgp_lgo_grad(ctx._h, 2, slots.ctypes.data_as(i32), th.ctypes.data_as(dbl), grp_.ctypes.data_as(i32) if grp_ is not None else None,
                                       ng_.ctypes.data_as(i32) if ng_ is not None else None, flag, obj.ctypes.data_as(dbl),
                                       grad_.ctypes.data_as(dbl) if grad_ is not None else None, None, None)

    bad = grp.copy()
    bad[5] = 3
    assert call(bad, ng, 1, grad) == -1          # id out of range
    bad[5] = -2
    assert call(bad, ng, 1, grad) == -1
    assert call(grp, None, 1, grad) == -1        # ngroups NULL with group
    assert call(grp, ng, 4, grad) == -1          # bad flag_grad bit
    assert call(grp, ng, 1, None) == -1          # grad NULL with flag_grad = 1
    assert all(v[1] == 0 for v in ctx.profile_read().values())      # no device work
    assert call(grp, ng, 1, grad) == 0           # the context is still usable
    ctx.close()
    from medgp_amd import synth
    fam = (7, 17, 3, 2)
    ctx = make_ctx(fam, c["pts"][2:3])
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.lgo_grad([0], synth.theta(1, 0, *fam)[None, :], [gs[0]])
    assert "error -1" in str(e.value) and "Q <= 16" in str(e.value)
    ctx.close()


def test_failed_patient_gets_nan_and_spares_its_batch_mates():
    """a patient without noise and with duplicated times fails every retry (as in test_loo_gpu.py)"""
    c = G.case("lmc_sizes")
    D = c["D"]
    sing = (np.zeros(6, np.int32), np.array([1, 1, 1, 2, 2, 2], np.float32), np.ones(6, np.float32))
    pts = [c["pts"][2], sing, c["pts"][4]]
    th = np.stack([c["th"][2], c["th"][3], c["th"][4]])
    th[1, :D] = -80.0
    gs = [G.groups_of(c, 2, "cov")[0], np.array([0, 0, 1, 1, 2, -1], np.int32), G.groups_of(c, 4, "cov")[0]]
    ctx = make_ctx(G.fam(c), pts, "pinned")
    obj, grad, st, gst = ctx.lgo_grad([0, 1, 2], th, gs)
    gobj, ggrad, gstt, _ = ctx.lgo_grad([0, 2], th[[0, 2]], [gs[0], gs[2]])
    obj0, _, st0, _ = ctx.lgo_grad([0, 1, 2], th, gs, False)
    ctx.close()
    assert st[1] == -1 and st0[1] == -1 and st[0] == 0 and st[2] == 0 and np.all(gstt == 0), (st, gstt)
    assert np.all(gst[1] == -1) and np.all(gst[0] == 0) and np.all(gst[2] == 0)
    assert np.isnan(obj[1]) and np.all(np.isnan(grad[1])) and np.isnan(obj0[1])
    assert np.array_equal(_bits(obj[[0, 2]]), _bits(gobj)) and np.array_equal(_bits(grad[[0, 2]]), _bits(ggrad))
    _assert_held([_hold(c, p, "cov", obj[i], grad[i], "beside a failure") for i, p in ((0, 2), (2, 4))])


def test_get_factor_after_the_call_is_that_of_nlml_grad():
    c = G.case("lmc_sizes")
    p = 5
    n = c["pts"][p][1].shape[0]
    th = c["th"][p][None, :]
    ctx = make_ctx(G.fam(c), [c["pts"][p]], "pinned")
    ctx.nlml_grad([0], th, False, keep_factor=True)
    a0, l0, b0 = ctx.get_factor(0, n)
    ctx.lgo_grad([0], th, [G.groups_of(c, p, "rand")[0]])
    a1, l1, b1 = ctx.get_factor(0, n)
    ctx.close()
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)) and np.array_equal(l0.view(np.uint32), l1.view(np.uint32)) and b0 == b1


def test_launch_counts_of_a_one_class_one_chunk_call():
    c = G.case("lmc_sizes")
    p = 5
    th = c["th"][p][None, :]
    grp = G.groups_of(c, p, "cov")[0]
    ctx = make_ctx(G.fam(c), [c["pts"][p]])
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.lgo_grad([0], th, [grp])
    full = {k: v[1] for k, v in ctx.profile_read().items()}
    ctx.profile_reset()
    ctx.lgo_grad([0], th, [grp], False)
    objonly = {k: v[1] for k, v in ctx.profile_read().items()}
    ctx.close()
    want = dict(k_loo_vec=2, k_lgo_vec=3, k_loo_kinv=1, k_loo_gram=1, k_postfactor=1, k_loo_solve=1, k_lgo_inv=1, k_lgo_s=1, k_lgo_t=1,
                k_lgo_wgrad=1, k_epilogue=2, k_wgrad=0, k_loo_wgrad=0, k_loo_diag=0)
    assert {k: full[k] for k in want} == want, full
    want0 = dict(k_loo_vec=1, k_lgo_vec=2, k_loo_kinv=0, k_loo_gram=1, k_postfactor=1, k_loo_solve=1, k_lgo_inv=0, k_lgo_s=0, k_lgo_t=0,
                 k_lgo_wgrad=0, k_epilogue=1)
    assert {k: objonly[k] for k in want0} == want0, objonly
    assert ctx._lib.medgp_profile_num_kernels() == 23
