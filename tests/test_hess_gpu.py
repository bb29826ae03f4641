"""medgp_hess_vec on the MI355X: the exact Hessian products against the long-double truth (hess_truth.py) within the fp64 budget
measured on CPU programs alone, for every size at which the kernels take another path and every family, on the default routing, the
pinned one-workgroup route and the look-ahead route; the gradient output; symmetry and the scale identity; the full matrix; bit
invariance (number and position of the directions, batch, upload order, prior); jitter retries; a failed patient; get_factor;
argument and capacity errors; launch counts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
from medgp_amd import curvature, information
import hess_truth as HT
import nlml_truth as T

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


def _hold(c, p, hv, what, jitter_rounds=0):
    """one patient's device products (NVEC directions) against the truth within the budget; prints the observed error"""
    tr, mg, bud = HT.budget_of(c, p, jitter_rounds)
    e = HT.errors(hv, tr, mg)
    print(f"HESS-ERR {what} {c['id']}:{p} n {c['pts'][p][1].shape[0]}: {e:.3g} (budget {bud:.3g})")
    return (what, c["id"], p, e, bud)


def _assert_held(rows):
    bad = [r for r in rows if not r[3] <= r[4]]
    assert not bad, bad


def _dirs(c, ps, nvec=HT.NVEC):
    return np.stack([HT.directions(c, p, nvec) for p in ps])


_GRAD_BUDGET = {}


def _grad_budget(c, p):
    """(truth gradient of L, budget): the nlml gradient budget of section 4.7d's method on the two fp64 programs of hess_truth -- (b)
    the truth's code in float64, (c) through numpy.linalg -- with M_GRAD, floored and capped as every gradient budget"""
    key = (c["id"], p)
    if key not in _GRAD_BUDGET:
        m, t, y = c["pts"][p]
        fam, th = HT.fam(c), c["th"][p]
        tg = HT.truth_of(c, p)[1]
        v0 = np.zeros((1, th.shape[0]))
        gb = HT.hess_vec(*fam, m, t, y, th, v0, np.float64, want_grad=True)[1]
        K = T.gram(*fam, m, np.asarray(t, np.float32), th, np.float64)
        Pc = np.linalg.inv(K)
        ac = np.linalg.solve(K, np.asarray(y, np.float32).astype(np.float64))
        gc = HT.hess_from_parts(*fam, m, t, th, (Pc + Pc.T) / 2, ac, v0, np.float64, "blocks")[1]
        eg = [HT.error_pair(1.0, gb, 1.0, tg)[1], HT.error_pair(1.0, gc, 1.0, tg)[1]]
        _GRAD_BUDGET[key] = (tg, min(HT.budget(eg, HT.LG.M_GRAD), HT.GRAD_BUDGET_CAP))
    return _GRAD_BUDGET[key]


# every case on the default and the pinned route; the look-ahead leg where the batch holds an entry of more than two 64-blocks
_LEGS = [(s[0], r) for s in HT.LG._SPECS for r in ROUTES if r != "la" or max(n for n, _ in s[5]) > 128]


@pytest.mark.parametrize("cid,route", _LEGS, ids=[f"{c}-{r}" for c, r in _LEGS])
def test_device_within_budget(cid, route, monkeypatch):
    """every case as one (ragged) batch in a shuffled order, two directions per patient; the gradient output within the nlml gradient
    budget.  la: the look-ahead factorisation forced for the entries that qualify (the knob is read when the context is created)"""
    c = HT.case(cid)
    P = len(c["pts"])
    if route == "la":
        monkeypatch.setenv("MEDGP_MULTI_CU", "1")
    order = np.array([5, 0, 3, 6, 1, 4, 2]) if P == 7 else np.arange(P)
    th = np.stack(c["th"])
    ctx = make_ctx(HT.fam(c), c["pts"], route)
    hv, g, st = ctx.hess_vec(order, th[order], _dirs(c, order), want_grad=True)
    ctx.close()
    assert np.all(st == 0), st
    rows = [_hold(c, p, hv[i], route) for i, p in enumerate(order)]
    for i, p in enumerate(order):
        tg, bud = _grad_budget(c, p)
        e = HT.error_pair(1.0, g[i], 1.0, tg)[1]
        print(f"HESS-GRAD-ERR {route} {cid}:{p}: {e:.3g} (budget {bud:.3g})")
        rows.append((route + "-grad", cid, p, e, bud))
    _assert_held(rows)


def test_symmetry_and_scale_identity():
    """u . H v against v . H u: each product is within its budget of the truth component by component, and the truth is symmetric.
    The scale identity s^T H s (+ g_A . vec(A)) = 2 y^T alpha: the left side is within budget of the truth's, which meets the
    right side (test_hess.py)."""
    for cid, ps in (("lmc_sizes", [2, 4, 5, 6]), ("sm_Q4", [0]), ("se", [0])):
        c = HT.case(cid)
        fam = HT.fam(c)
        th = np.stack([c["th"][p] for p in ps])
        V = _dirs(c, ps)
        S = np.stack([information.scale_direction(*fam, t_) for t_ in th])
        ctx = make_ctx(fam, [c["pts"][p] for p in ps])
        hv, g, st = ctx.hess_vec(np.arange(len(ps)), th, np.concatenate([V, S[:, None, :]], axis=1), want_grad=True)
        ctx.close()
        assert np.all(st == 0)
        for i, p in enumerate(ps):
            m, t, y = c["pts"][p]
            tr, mg, bud = HT.budget_of(c, p)
            sc = [HT.scale_of(mg[j]).astype(np.float64) for j in range(2)]
            a, b = float(V[i, 0] @ hv[i, 1]), float(V[i, 1] @ hv[i, 0])
            bound = bud * float(np.abs(V[i, 0]) @ sc[1] + np.abs(V[i, 1]) @ sc[0])
            print(f"HESS-SYM {cid}:{p}: |uHv - vHu| = {abs(a - b):.3g} (bound {bound:.3g}, uHv {a:.6g})")
            assert abs(a - b) <= bound, (p, a, b, bound)
            Pm, alpha, _ = HT.parts(*fam, m, t, y, th[i], X)
            hs, tg, smag = HT.hess_from_parts(*fam, m, t, th[i], Pm, alpha, S[i], X, want_mag=True)
            want = float(2 * np.sum(np.asarray(y, np.float32).astype(X) * alpha))
            got = float(HT.scale_identity(fam, th[i], S[i], hv[i, 2], g[i]))
            ssc = HT.scale_of(smag[0]).astype(np.float64)
            gsc = np.maximum(np.abs(tg), 1e-3 * np.abs(tg).max()).astype(np.float64)
            gb = _grad_budget(c, p)[1]
            bound = bud * float(np.abs(S[i]) @ ssc) + (gb * float(np.abs(th[i]) @ gsc) if fam[0] == 7 else 0.0) + 64 * HT.COND_MAX * 2.0 ** -53 * abs(want)
            print(f"HESS-SCALE {cid}:{p}: sHs (+ gA) {got:.9g}, 2 y alpha {want:.9g} (bound {bound:.3g})")
            assert abs(got - want) <= bound, (p, got, want, bound)


def test_full_matrix_of_the_n63_lmc_case():
    """information.fisher_matrix through curvature.bind (H = 25 unit directions in one call) against the truth's matrix, entry by
    entry: every entry of a product is within the budget on the scale of its row or column (hess_truth.scale_of)"""
    c = HT.case("lmc_sizes")
    p = 2
    m, t, y = c["pts"][p]
    H = c["th"][p].shape[0]
    assert H == 25
    ctx = make_ctx(HT.fam(c), [c["pts"][p]])
    Hm = information.fisher_matrix(curvature.bind(ctx, [0], c["th"][p][None, :]), H)[0]
    ctx.close()
    Ht, Hmag = HT.hess_vec(*HT.fam(c), m, t, y, c["th"][p], np.eye(H), X, want_mag=True)
    Ht = ((Ht + Ht.T) / 2).astype(np.float64)
    _, _, bud = HT.budget_of(c, p)
    scale = np.stack([HT.scale_of(r) for r in Hmag]).astype(np.float64)
    worst = float((np.abs(Hm - Ht) / np.maximum(scale, scale.T)).max())
    print(f"HESS-MATRIX worst entry error {worst:.3g} (budget {bud:.3g}), eigenvalues {np.linalg.eigvalsh(Hm)[[0, -1]]}")
    assert worst <= bud


def test_bits():
    """route pinned: a direction's bits depend on the patient, theta and the direction alone"""
    c = HT.case("lmc_sizes")
    P = len(c["pts"])
    th = np.stack(c["th"])
    H = th.shape[1]
    V3 = _dirs(c, range(P), 3)
    m5, t5, y5 = c["pts"][5]
    # the covariates interleaved at random, every covariate's observations in the order of the grouped upload: the library groups
    # stably, so the patient it works on is the grouped one, row for row
    g = T._philox(20261406, 0)
    keys = g.random(m5.shape[0])
    for d in range(c["D"]):
        keys[m5 == d] = np.sort(keys[m5 == d])
    perm = np.argsort(keys, kind="stable")
    assert np.any(np.diff(m5[perm]) < 0) and all(np.array_equal(perm[m5[perm] == d], np.flatnonzero(m5 == d)) for d in range(c["D"]))
    shuf = g.permutation(m5.shape[0])
    pts = c["pts"] + [(m5[perm], t5[perm], y5[perm]), (m5[shuf], t5[shuf], y5[shuf])]
    ctx = make_ctx(HT.fam(c), pts, "pinned")
    slots = np.arange(P)
    h3, g3, st = ctx.hess_vec(slots, th, V3, want_grad=True)
    assert np.all(st == 0) and h3.shape == (P, 3, H) and g3.shape == (P, H)
    h1, _ = ctx.hess_vec(slots, th, V3[:, 1])                           # nvec = 1 against 3, [nbatch, H] in and out, no gradient
    assert h1.shape == (P, H) and np.array_equal(_bits(h1), _bits(h3[:, 1]))
    hm, _ = ctx.hess_vec(slots, th, V3[:, [2, 0, 1]])                   # every direction at another position
    assert np.array_equal(_bits(hm), _bits(h3[:, [2, 0, 1]]))
    hr, gr, _ = ctx.hess_vec(slots[::-1].copy(), th[::-1].copy(), V3[::-1].copy(), want_grad=True)      # the batch of 7 reversed
    assert np.array_equal(_bits(hr[::-1]), _bits(h3)) and np.array_equal(_bits(gr[::-1]), _bits(g3))
    for p in range(P):                                                  # alone
        ha, ga, _ = ctx.hess_vec([p], th[p:p + 1], V3[p:p + 1], want_grad=True)
        assert np.array_equal(_bits(ha[0]), _bits(h3[p])) and np.array_equal(_bits(ga[0]), _bits(g3[p])), p
    ho, sto = ctx.hess_vec([P, 2, P + 1], th[[5, 2, 5]], V3[[5, 2, 5]])
    assert np.all(sto == 0)
    assert np.array_equal(_bits(ho[0]), _bits(h3[5]))                   # covariates interleaved on upload: the grouped upload's result
    _assert_held([_hold(c, 5, ho[2, :HT.NVEC], "shuffled upload")])     # another order inside a covariate: held to the budget
    flag = np.ones(H, np.uint8)
    typ = np.full(H, 1, np.int32)
    typ[[2, 7]] = 0                                                     # two clamps, normal priors elsewhere
    ctx.set_prior(-1, flag, typ, np.zeros(H, np.uint8), np.full(H, 0.3, np.float32), np.full(H, 0.5, np.float32))
    hp, gp, stp = ctx.hess_vec(slots, th, V3, want_grad=True)
    ctx.close()
    assert np.all(stp == 0) and np.array_equal(_bits(hp), _bits(h3)) and np.array_equal(_bits(gp), _bits(g3))   # a prior on every slot changes nothing


_CHILD = """
import sys
import numpy as np
import medgp_amd
import hess_truth as HT
c = HT.case("lmc_sizes")
ps = [2, 4, 5]
ctx = medgp_amd.Context(*HT.fam(c))
ctx.reserve(3, 130, 3)
for s, p in enumerate(ps):
    ctx.set_patient(s, *c["pts"][p])
hv, st = ctx.hess_vec([0, 1, 2], np.stack([c["th"][p] for p in ps]), np.stack([HT.directions(c, p) for p in ps]))
ctx.close()
np.savez(sys.argv[1], hv=hv, st=st)
"""


@pytest.mark.parametrize("fails", [1, 3])
def test_jitter_retries(fails, tmp_path):
    """P and alpha are those of the matrix that was factored, K + k diag(sigma^2), the kernel derivatives un-jittered; the hook is read
    when the library creates a context, in a process of its own"""
    env = dict(os.environ, MEDGP_DEBUG_FAIL_ATTEMPTS=str(fails), PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    out = str(tmp_path / "jitter.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert np.all(z["st"] == fails), z["st"]
    c = HT.case("lmc_sizes")
    _assert_held([_hold(c, p, z["hv"][i], f"jitter{fails}", fails) for i, p in enumerate([2, 4, 5])])


def test_failed_patient_gets_nan_and_spares_its_batch_mates():
    """a patient without noise and with duplicated times fails every retry (as in test_loo_gpu.py)"""
    c = HT.case("lmc_sizes")
    D = c["D"]
    sing = (np.zeros(6, np.int32), np.array([1, 1, 1, 2, 2, 2], np.float32), np.ones(6, np.float32))
    pts = [c["pts"][2], sing, c["pts"][4]]
    th = np.stack([c["th"][2], c["th"][3], c["th"][4]])
    th[1, :D] = -80.0
    V = _dirs(c, [2, 3, 4])
    ctx = make_ctx(HT.fam(c), pts, "pinned")
    hv, g, st = ctx.hess_vec([0, 1, 2], th, V, want_grad=True)
    h2, g2, st2 = ctx.hess_vec([0, 2], th[[0, 2]], V[[0, 2]], want_grad=True)
    ctx.close()
    assert st[1] == -1 and st[0] == 0 and st[2] == 0 and np.all(st2 == 0), (st, st2)
    assert np.all(np.isnan(hv[1])) and np.all(np.isnan(g[1]))
    assert np.array_equal(_bits(hv[[0, 2]]), _bits(h2)) and np.array_equal(_bits(g[[0, 2]]), _bits(g2))
    _assert_held([_hold(c, p, hv[i], "beside a failure") for i, p in ((0, 2), (2, 4))])


def test_get_factor_after_the_call_is_that_of_nlml_grad():
    c = HT.case("lmc_sizes")
    p = 5
    n = c["pts"][p][1].shape[0]
    th = c["th"][p][None, :]
    ctx = make_ctx(HT.fam(c), [c["pts"][p]], "pinned")
    ctx.nlml_grad([0], th, False, keep_factor=True)
    a0, l0, b0 = ctx.get_factor(0, n)
    ctx.hess_vec([0], th, _dirs(c, [p]))
    a1, l1, b1 = ctx.get_factor(0, n)
    ctx.close()
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)) and np.array_equal(l0.view(np.uint32), l1.view(np.uint32)) and b0 == b1


def test_argument_errors():
    c = HT.case("lmc_sizes")
    ctx = make_ctx(HT.fam(c), c["pts"][2:4])
    th = np.stack(c["th"][2:4])
    V = _dirs(c, [2, 3])
    H = th.shape[1]
    ctx.profile_enable(True)
    ctx.profile_reset()
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.hess_vec([0, 1], th, np.zeros((2, 0, H)))
    assert "error -1" in str(e.value) and "nvec" in str(e.value)
    slots = np.arange(2, dtype=np.int32)
    out = np.zeros_like(V)
    i32, dbl = C.POINTER(C.c_int32), C.POINTER(C.c_double)

    def call(s, t, nvec, v, o):
        ptr = lambda a, ty: a.ctypes.data_as(ty) if a is not None else None
        return ctx._lib.medgp_hess_vec(ctx._h, 2, ptr(s, i32), ptr(t, dbl), nvec, ptr(v, dbl), ptr(o, dbl), None, None)

    assert call(slots, th, 0, V, out) == -1
    assert call(slots, th, -3, V, out) == -1
    assert call(None, th, 2, V, out) == -1
    assert call(slots, None, 2, V, out) == -1
    assert call(slots, th, 2, None, out) == -1
    assert call(slots, th, 2, V, None) == -1
    assert all(v[1] == 0 for v in ctx.profile_read().values())      # no device work
    assert call(slots, th, 2, V, out) == 0                          # the context is still usable (grad and status NULL)
    ctx.close()
    from medgp_amd import synth
    fam = (7, 17, 3, 2)
    ctx = make_ctx(fam, c["pts"][2:3])
    th17 = synth.theta(1, 0, *fam)[None, :]
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.hess_vec([0], th17, np.ones_like(th17))
    assert "error -1" in str(e.value) and "Q <= 16" in str(e.value)
    ctx.close()


def test_capacity_error(monkeypatch):
    """four 256 x 256 matrices of doubles for the n = 200 patient are 2 MiB: a budget of 1.5 MiB holds the two the factorisation
    needs (so medgp_loo_grad runs) and refuses this call; the budget is read when the context is created"""
    monkeypatch.setenv("MEDGP_MEM_BUDGET_GB", repr(1.5 / 1024))
    c = HT.case("lmc_sizes")
    ctx = make_ctx(HT.fam(c), [c["pts"][6]])
    th = c["th"][6][None, :]
    _, _, st = ctx.loo_grad([0], th)
    assert st[0] == 0
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.hess_vec([0], th, _dirs(c, [6]))
    assert "MEDGP_MEM_BUDGET_GB" in str(e.value) and "-4" in str(e.value)   # MEDGP_ERR_CAPACITY
    ctx.close()


def test_launch_counts_of_a_one_class_call():
    """nvec = 2, one size class, Q <= 8: k_loo_kinv, the moment pass and its two slab sums once; per direction one launch of each of
    the six kernels plus k_slabsum (counted under k_epilogue, with the W pass's k_slabsum: 3; with the gradient output's k_epilogue: 4)"""
    c = HT.case("lmc_sizes")
    p = 5
    ctx = make_ctx(HT.fam(c), [c["pts"][p]])
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.hess_vec([0], c["th"][p][None, :], _dirs(c, [p]))
    got = {k: v[1] for k, v in ctx.profile_read().items()}
    ctx.profile_reset()
    ctx.hess_vec([0], c["th"][p][None, :], _dirs(c, [p]), want_grad=True)
    got_g = {k: v[1] for k, v in ctx.profile_read().items()}
    ctx.close()
    want = dict(k_prep=1, k_assemble=1, k_loo_kinv=1, k_hess_moments=1, k_hess_slabsum=1, k_fisher_prep=2, k_fisher_kdot=2, k_fisher_t=2,
                k_hess_beta=2, k_hess_wgrad=2, k_hess_epilogue=2, k_epilogue=3, k_wgrad=0, k_fisher_wgrad=0, k_loo_wgrad=0, k_loo_vec=0,
                k_lgo_wgrad=0)
    assert {k: got[k] for k in want} == want, got
    assert {k: got_g[k] for k in want} == dict(want, k_epilogue=4), got_g
    assert ctx._lib.medgp_profile_num_kernels() == 23 and ctx._lib.medgp_profile_num_kernels_all() == 29
