"""medgp_fisher_vec on the MI355X: the Fisher-information products against the long-double truth (fisher_truth.py) within the fp64
budget measured on CPU programs alone, for every size at which the kernels take another path and every family, on the default
routing, the pinned one-workgroup route and the look-ahead route; the scale direction; symmetry; bit invariance (number and position
of the directions, batch, upload order, y, prior); jitter retries; a failed patient; get_factor; argument and capacity errors; the
full matrix; launch counts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
from medgp_amd import information
import fisher_truth as F

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


def _hold(c, p, fv, what, jitter_rounds=0):
    """one patient's device products (NVEC directions) against the truth within the budget; prints the observed error"""
    tr, bud = F.budget_of(c, p, jitter_rounds)
    e = F.errors(fv, tr)
    print(f"FISHER-ERR {what} {c['id']}:{p} n {c['pts'][p][1].shape[0]}: {e:.3g} (budget {bud:.3g})")
    return (what, c["id"], p, e, bud)


def _assert_held(rows):
    bad = [r for r in rows if not r[3] <= r[4]]
    assert not bad, bad


def _dirs(c, ps, nvec=F.NVEC):
    return np.stack([F.directions(c, p, nvec) for p in ps])


# every case on the default and the pinned route; the look-ahead leg where the batch holds an entry of more than two 64-blocks
_LEGS = [(s[0], r) for s in F.LG._SPECS for r in ROUTES if r != "la" or max(n for n, _ in s[5]) > 128]


@pytest.mark.parametrize("cid,route", _LEGS, ids=[f"{c}-{r}" for c, r in _LEGS])
def test_device_within_budget(cid, route, monkeypatch):
    """every case as one (ragged) batch, two directions per patient.  la: the look-ahead factorisation forced for the entries that
    qualify (the knob is read when the context is created)"""
    c = F.case(cid)
    P = len(c["pts"])
    if route == "la":
        monkeypatch.setenv("MEDGP_MULTI_CU", "1")
    order = np.array([5, 0, 3, 6, 1, 4, 2]) if P == 7 else np.arange(P)
    th = np.stack(c["th"])
    ctx = make_ctx(F.fam(c), c["pts"], route)
    fv, st = ctx.fisher_vec(order, th[order], _dirs(c, order))
    ctx.close()
    assert np.all(st == 0), st
    _assert_held([_hold(c, p, fv[i], route) for i, p in enumerate(order)])


def test_scale_direction():
    """s^T (F s) = 2 n: along s Kdot = 2 K, so W_F = 2 P and the products with P K = I.  To 64 n 2^-53 relative."""
    rows = []
    for cid in ("lmc_sizes", "sm_Q4", "se"):
        c = F.case(cid)
        P = len(c["pts"])
        th = np.stack(c["th"])
        s = np.stack([information.scale_direction(*F.fam(c), th[p]) for p in range(P)])
        ctx = make_ctx(F.fam(c), c["pts"])
        fs, st = ctx.fisher_vec(np.arange(P), th, s)
        ctx.close()
        assert np.all(st == 0) and fs.shape == s.shape
        for p in range(P):
            n = c["pts"][p][1].shape[0]
            got = float(np.sum(s[p].astype(X) * fs[p].astype(X)))
            rows.append((cid, p, n, abs(got - 2 * n) / (2 * n), 64 * n * 2.0 ** -53))
            print(f"FISHER-SCALE {cid}:{p} n {n}: |sFs - 2n| / 2n = {rows[-1][3]:.3g} (bound {rows[-1][4]:.3g})")
    bad = [r for r in rows if not r[3] <= r[4]]
    assert not bad, bad


def test_symmetry():
    """u . F v against v . F u: each product is within its budget of the truth component by component, and the truth is symmetric"""
    c = F.case("lmc_sizes")
    ps = [2, 4, 5, 6]
    ctx = make_ctx(F.fam(c), [c["pts"][p] for p in ps])
    V = _dirs(c, ps)
    fv, st = ctx.fisher_vec(np.arange(4), np.stack([c["th"][p] for p in ps]), V)
    ctx.close()
    assert np.all(st == 0)
    for i, p in enumerate(ps):
        tr, bud = F.budget_of(c, p)
        sc = [np.maximum(np.abs(tr[j]), 1e-3 * np.abs(tr[j]).max()).astype(np.float64) for j in range(2)]
        a, b = float(V[i, 0] @ fv[i, 1]), float(V[i, 1] @ fv[i, 0])
        bound = bud * float(np.abs(V[i, 0]) @ sc[1] + np.abs(V[i, 1]) @ sc[0])
        print(f"FISHER-SYM lmc_sizes:{p}: |uFv - vFu| = {abs(a - b):.3g} (bound {bound:.3g}, uFv {a:.6g})")
        assert abs(a - b) <= bound, (p, a, b, bound)
        assert float(V[i, 0] @ fv[i, 0]) > 0 and float(V[i, 1] @ fv[i, 1]) > 0


def test_bits():
    """route pinned: a direction's bits depend on the patient, theta and the direction alone"""
    c = F.case("lmc_sizes")
    P = len(c["pts"])
    th = np.stack(c["th"])
    H = th.shape[1]
    V3 = _dirs(c, range(P), 3)
    m5, t5, y5 = c["pts"][5]
    # the covariates interleaved at random, every covariate's observations in the order of the grouped upload: the library groups
    # stably, so the patient it works on is the grouped one, row for row.  (Another order INSIDE a covariate is another order of
    # every sum: such an upload is held to the budget below, not to the bits.)
    g = F.T._philox(20261305, 0)
    keys = g.random(m5.shape[0])
    for d in range(c["D"]):
        keys[m5 == d] = np.sort(keys[m5 == d])
    perm = np.argsort(keys, kind="stable")
    assert np.any(np.diff(m5[perm]) < 0) and all(np.array_equal(perm[m5[perm] == d], np.flatnonzero(m5 == d)) for d in range(c["D"]))
    shuf = g.permutation(m5.shape[0])
    pts = c["pts"] + [(m5[perm], t5[perm], y5[perm]), (m5, t5, (3 * y5[::-1] + 1).astype(np.float32)), (m5[shuf], t5[shuf], y5[shuf])]
    ctx = make_ctx(F.fam(c), pts, "pinned")
    slots = np.arange(P)
    f3, st = ctx.fisher_vec(slots, th, V3)
    assert np.all(st == 0) and f3.shape == (P, 3, H)
    f1, _ = ctx.fisher_vec(slots, th, V3[:, 1])                        # nvec = 1 against 3, [nbatch, H] in and out
    assert f1.shape == (P, H) and np.array_equal(_bits(f1), _bits(f3[:, 1]))
    fm, _ = ctx.fisher_vec(slots, th, V3[:, [2, 0, 1]])                # every direction at another position
    assert np.array_equal(_bits(fm), _bits(f3[:, [2, 0, 1]]))
    fr, _ = ctx.fisher_vec(slots[::-1].copy(), th[::-1].copy(), V3[::-1].copy())      # another batch order
    assert np.array_equal(_bits(fr[::-1]), _bits(f3))
    for p in range(P):                                                 # other batch-mates: none
        fa, _ = ctx.fisher_vec([p], th[p:p + 1], V3[p:p + 1])
        assert np.array_equal(_bits(fa[0]), _bits(f3[p])), p
    fo, sto = ctx.fisher_vec([P, P + 1, 2, P + 2], th[[5, 5, 2, 5]], V3[[5, 5, 2, 5]])
    assert np.all(sto == 0)
    _assert_held([_hold(c, 5, fo[3, :F.NVEC], "shuffled upload")])
    assert np.array_equal(_bits(fo[0]), _bits(f3[5]))                  # uploaded in caller order: the grouped upload's result
    assert np.array_equal(_bits(fo[1]), _bits(f3[5]))                  # another y
    flag = np.ones(H, np.uint8)
    typ = np.full(H, 1, np.int32)
    typ[[2, 7]] = 0                                                    # two clamps, normal priors elsewhere
    ctx.set_prior(-1, flag, typ, np.zeros(H, np.uint8), np.full(H, 0.3, np.float32), np.full(H, 0.5, np.float32))
    fp, stp = ctx.fisher_vec(slots, th, V3)
    ctx.close()
    assert np.all(stp == 0) and np.array_equal(_bits(fp), _bits(f3))   # a prior on every slot changes nothing


_CHILD = """
import sys
import numpy as np
import medgp_amd
import fisher_truth as F
c = F.case("lmc_sizes")
ps = [2, 4, 5]
ctx = medgp_amd.Context(*F.fam(c))
ctx.reserve(3, 130, 3)
for s, p in enumerate(ps):
    ctx.set_patient(s, *c["pts"][p])
fv, st = ctx.fisher_vec([0, 1, 2], np.stack([c["th"][p] for p in ps]), np.stack([F.directions(c, p) for p in ps]))
ctx.close()
np.savez(sys.argv[1], fv=fv, st=st)
"""


@pytest.mark.parametrize("fails", [1, 3])
def test_jitter_retries(fails, tmp_path):
    """P is the inverse of the matrix that was factored, K + k diag(sigma^2), Kdot the un-jittered derivative; the hook is read when
    the library creates a context, in a process of its own"""
    env = dict(os.environ, MEDGP_DEBUG_FAIL_ATTEMPTS=str(fails), PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    out = str(tmp_path / "jitter.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert np.all(z["st"] == fails), z["st"]
    c = F.case("lmc_sizes")
    _assert_held([_hold(c, p, z["fv"][i], f"jitter{fails}", fails) for i, p in enumerate([2, 4, 5])])


def test_failed_patient_gets_nan_and_spares_its_batch_mates():
    """a patient without noise and with duplicated times fails every retry (as in test_loo_gpu.py)"""
    c = F.case("lmc_sizes")
    D = c["D"]
    sing = (np.zeros(6, np.int32), np.array([1, 1, 1, 2, 2, 2], np.float32), np.ones(6, np.float32))
    pts = [c["pts"][2], sing, c["pts"][4]]
    th = np.stack([c["th"][2], c["th"][3], c["th"][4]])
    th[1, :D] = -80.0
    V = _dirs(c, [2, 3, 4])
    ctx = make_ctx(F.fam(c), pts, "pinned")
    fv, st = ctx.fisher_vec([0, 1, 2], th, V)
    gv, gst = ctx.fisher_vec([0, 2], th[[0, 2]], V[[0, 2]])
    ctx.close()
    assert st[1] == -1 and st[0] == 0 and st[2] == 0 and np.all(gst == 0), (st, gst)
    assert np.all(np.isnan(fv[1]))
    assert np.array_equal(_bits(fv[[0, 2]]), _bits(gv))
    _assert_held([_hold(c, p, fv[i], "beside a failure") for i, p in ((0, 2), (2, 4))])


def test_get_factor_after_the_call_is_that_of_nlml_grad():
    c = F.case("lmc_sizes")
    p = 5
    n = c["pts"][p][1].shape[0]
    th = c["th"][p][None, :]
    ctx = make_ctx(F.fam(c), [c["pts"][p]], "pinned")
    ctx.nlml_grad([0], th, False, keep_factor=True)
    a0, l0, b0 = ctx.get_factor(0, n)
    ctx.fisher_vec([0], th, _dirs(c, [p]))
    a1, l1, b1 = ctx.get_factor(0, n)
    ctx.close()
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)) and np.array_equal(l0.view(np.uint32), l1.view(np.uint32)) and b0 == b1


def test_argument_errors():
    c = F.case("lmc_sizes")
    ctx = make_ctx(F.fam(c), c["pts"][2:4])
    th = np.stack(c["th"][2:4])
    V = _dirs(c, [2, 3])
    H = th.shape[1]
    ctx.profile_enable(True)
    ctx.profile_reset()
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.fisher_vec([0, 1], th, np.zeros((2, 0, H)))
    assert "error -1" in str(e.value) and "nvec" in str(e.value)
    slots = np.arange(2, dtype=np.int32)
    out = np.zeros_like(V)
    i32, dbl = C.POINTER(C.c_int32), C.POINTER(C.c_double)

    def call(s, t, nvec, v, o):
        ptr = lambda a, ty: a.ctypes.data_as(ty) if a is not None else None
        return ctx._lib.medgp_fisher_vec(ctx._h, 2, ptr(s, i32), ptr(t, dbl), nvec, ptr(v, dbl), ptr(o, dbl), None)

    assert call(slots, th, 0, V, out) == -1
    assert call(slots, th, -3, V, out) == -1
    assert call(None, th, 2, V, out) == -1
    assert call(slots, None, 2, V, out) == -1
    assert call(slots, th, 2, None, out) == -1
    assert call(slots, th, 2, V, None) == -1
    assert all(v[1] == 0 for v in ctx.profile_read().values())      # no device work
    assert call(slots, th, 2, V, out) == 0                          # the context is still usable
    ctx.close()
    from medgp_amd import synth
    fam = (7, 17, 3, 2)
    ctx = make_ctx(fam, c["pts"][2:3])
    th17 = synth.theta(1, 0, *fam)[None, :]
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.fisher_vec([0], th17, np.ones_like(th17))
    assert "error -1" in str(e.value) and "Q <= 16" in str(e.value)
    ctx.close()


def test_capacity_error(monkeypatch):
    """four 256 x 256 matrices of doubles for the n = 200 patient are 2 MiB: a budget of 1.5 MiB holds the two the factorisation
    needs (so medgp_loo_grad runs) and refuses this call; the budget is read when the context is created"""
    monkeypatch.setenv("MEDGP_MEM_BUDGET_GB", repr(1.5 / 1024))
    c = F.case("lmc_sizes")
    ctx = make_ctx(F.fam(c), [c["pts"][6]])
    th = c["th"][6][None, :]
    _, _, st = ctx.loo_grad([0], th)
    assert st[0] == 0
    with pytest.raises(medgp_amd.MedgpError) as e:
        ctx.fisher_vec([0], th, _dirs(c, [6]))
    assert "MEDGP_MEM_BUDGET_GB" in str(e.value) and "-4" in str(e.value)   # MEDGP_ERR_CAPACITY
    ctx.close()


def test_full_matrix_of_the_n63_lmc_case():
    """information.fisher_matrix through a bound context (H = 25 unit directions in one call) against the truth's matrix; every entry of
    a product is within the budget on the gradient scale of its column, and F is positive semi-definite to that accuracy"""
    c = F.case("lmc_sizes")
    p = 2
    m, t, _ = c["pts"][p]
    H = c["th"][p].shape[0]
    assert H == 25
    ctx = make_ctx(F.fam(c), [c["pts"][p]])
    Fm = information.fisher_matrix(information.bind(ctx, [0], c["th"][p][None, :]), H)[0]
    ctx.close()
    Ft = F.fisher_vec(*F.fam(c), m, t, c["th"][p], np.eye(H), X)
    Ft = ((Ft + Ft.T) / 2).astype(np.float64)
    _, bud = F.budget_of(c, p)
    scale = np.maximum(np.abs(Ft), 1e-3 * np.abs(Ft).max(axis=1, keepdims=True))
    worst = float((np.abs(Fm - Ft) / np.maximum(scale, scale.T)).max())
    lo = float(np.linalg.eigvalsh(Fm).min())
    nrm = float(np.linalg.norm(Fm, 2))
    print(f"FISHER-MATRIX worst entry error {worst:.3g} (budget {bud:.3g}), smallest eigenvalue {lo:.3g}, ||F|| {nrm:.3g}")
    assert worst <= bud
    assert lo >= -bud * nrm


def test_launch_counts_of_a_one_class_call():
    """nvec = 2, one size class, Q <= 8: one k_loo_kinv, and per direction one launch of each of the four kernels plus k_slabsum and
    k_epilogue (both counted under k_epilogue); the pipeline run before them ends without an epilogue"""
    c = F.case("lmc_sizes")
    p = 5
    ctx = make_ctx(F.fam(c), [c["pts"][p]])
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.fisher_vec([0], c["th"][p][None, :], _dirs(c, [p]))
    got = {k: v[1] for k, v in ctx.profile_read().items()}
    ctx.close()
    want = dict(k_prep=1, k_assemble=1, k_loo_kinv=1, k_fisher_prep=2, k_fisher_kdot=2, k_fisher_t=2, k_fisher_wgrad=2, k_epilogue=4,
                k_wgrad=0, k_loo_wgrad=0, k_loo_vec=0, k_lgo_wgrad=0)
    assert {k: got[k] for k in want} == want, got
    assert ctx._lib.medgp_profile_num_kernels() == 23 and ctx._lib.medgp_profile_num_kernels_all() == 29
