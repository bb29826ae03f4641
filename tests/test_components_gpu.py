"""medgp_components_batch on the MI355X: parity with the numpy definition (components_ref.py) on the inputs of components_cases.py --
the three covariance families, Q from 1 to 64, point counts on and around the tile width 64 / Q, every factorisation route -- the
invariants of a covariance block, consistency with medgp_posterior_batch on the same call, jitter rounds and failed entries, the bits
of a point's outputs (unchanged by the points' order, the split of a call and the launch chunks), the far field and the argument
errors.  Every parity test prints its worst error per quantity in fp32 ulps (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
from medgp_amd import synth
import components_cases as CC
import components_ref as CR
import posterior_ref as PR


def make_ctx(kidx, Q, D, R, pts):
    ctx = medgp_amd.Context(kidx, Q, D, R)
    ctx.reserve(len(pts), max(max(p[1].shape[0] for p in pts), 1), len(pts))
    for s, (m, t, y) in enumerate(pts):
        ctx.set_patient(s, m if kidx == 7 else None, t, y)
    return ctx


def check_case(name, fam, out, sel=None, who=""):
    """out[i] of patient sel[i] against the shared reference; prints the worst error per quantity"""
    sel = CC.checked(name) if sel is None else sel
    worst = [0.0] * 3
    for i, p in enumerate(sel):
        u = CR.check_components(fam[1], CC.case_ref(name, p), out[i])
        worst = [max(a, b) for a, b in zip(worst, u)]
    print(f"{name}{who}: " + " ".join(f"{n} {x:.3f}" for n, x in zip(CR.NAMES, worst)) + " (fp32 ulps)")


def check_sums(fam, th, qs, out, post):
    """the components of a point against medgp_posterior_batch on the same call, with the constant of check_posterior's parts rule:
        |sum_q cmean - mean| <= 4e-7 (Q + 1) (max|cmean| + |mean|),   |sum_qr ccov + sigma^2 - var| <= 4e-7 (Q^2 + 1) (max|ccov| + var)"""
    kidx, Q, D, _ = fam
    for p in range(len(out)):
        cmean, cvar, ccov = (a.astype(np.float64) for a in out[p])
        m = cmean.shape[0]
        if m == 0:
            continue
        mean, var = post[p][0].astype(np.float64), post[p][1].astype(np.float64)
        sig2 = PR.noise_var(kidx, D, th[p], qs[p][0] if kidx == 7 else np.zeros(m, np.int32))
        assert np.all(np.abs(cmean.sum(axis=1) - mean) <= 4e-7 * (Q + 1) * (np.abs(cmean).max() + np.abs(mean))), ("mean", p)
        assert np.all(np.abs(ccov.sum(axis=(1, 2)) + sig2 - var) <= 4e-7 * (Q * Q + 1) * (np.abs(ccov).max() + var)), ("var", p)


def run_case(name, with_posterior=False):
    fam, pts, th, qs = CC.case_data(name)
    ctx = make_ctx(*fam, pts)
    m2s, t2s = CC.call_lists(fam, qs)
    out, st = ctx.components(np.arange(len(pts)), th, m2s, t2s)
    plan = ctx.last_plan()
    if with_posterior:
        post, pst = ctx.posterior(np.arange(len(pts)), th, m2s, t2s, parts=False)
        assert np.array_equal(pst, st)
        check_sums(fam, th, qs, out, post)
    ctx.close()
    return fam, pts, th, qs, out, st, plan


@pytest.mark.parametrize("name", ["parity_d3", "parity_d24"])
def test_parity_with_definition_and_consistency_with_posterior(name):
    fam, pts, th, qs, out, st, _ = run_case(name, True)   # interleaved upload: the callers' order, not grouped
    assert np.all(st == 0)
    check_case(name, fam, out)


@pytest.mark.parametrize("name", ["tile_edges_q3", "tile_edges_q2"])
def test_tile_edges(name):
    fam, pts, th, qs, out, st, _ = run_case(name, True)
    Q = fam[1]
    assert np.all(st == 0)
    for p, k in enumerate(CC.CASES[name][6]):
        assert out[p][0].shape == (k, Q) and out[p][1].shape == (k, Q) and out[p][2].shape == (k, Q, Q)
    check_case(name, fam, out)


@pytest.mark.parametrize("name", ["q17", "q64", "se", "sm"])
def test_many_components_and_single_output_families(name):
    fam, pts, th, qs, out, st, _ = run_case(name, True)   # (se / sm: meta2 = None)
    assert np.all(st == 0)
    check_case(name, fam, out)


def test_routes_all_three_and_pinned():
    """One call whose size classes take the 4-wave (route 0), 8-wave (1) and look-ahead (2) factorisations."""
    fam, pts, th, qs = CC.case_data("routes")
    chk = CC.ROUTE_CHECKED
    ctx = make_ctx(*fam, pts)
    m2s, t2s = CC.call_lists(fam, qs)
    out, st = ctx.components(np.arange(len(pts)), th, m2s, t2s)
    assert {r for (_, _, r) in ctx.last_plan()} == {0, 1, 2}, ctx.last_plan()
    assert np.all(st == 0)
    assert all(out[p][0].shape == (0, fam[1]) for p in range(len(pts)) if p not in chk)
    check_case("routes", fam, [out[p] for p in chk], chk)
    ctx.pin_route(True)
    m2c, t2c = CC.call_lists(fam, qs, chk)
    out2, st2 = ctx.components(chk, th[chk], m2c, t2c)
    assert {r for (_, _, r) in ctx.last_plan()} == {1}
    assert np.all(st2 == 0)
    check_case("routes", fam, out2, chk, " pinned")
    ctx.close()


def test_forced_multi_cu_route(monkeypatch):
    monkeypatch.setenv("MEDGP_MULTI_CU", "1")
    fam, pts, th, qs, out, st, plan = run_case("multi_cu")
    assert {r for (_, _, r) in plan} == {2}
    assert np.all(st == 0)
    check_case("multi_cu", fam, out)


def test_jitter_rounds(monkeypatch):
    """MEDGP_DEBUG_FAIL_ATTEMPTS = 2: every quantity is that of the factor of K + 2 diag(sigma^2) (restate(jitter_rounds = 2))"""
    monkeypatch.setenv("MEDGP_DEBUG_FAIL_ATTEMPTS", str(CC.JITTER_ROUNDS["jitter"]))
    fam, pts, th, qs, out, st, _ = run_case("jitter")
    assert np.all(st == CC.JITTER_ROUNDS["jitter"]), st
    check_case("jitter", fam, out)


def test_failed_entry_gives_nan_and_spares_batch_mates():
    fam, pts, th, qs = CC.case_data("jitter")
    Q, D = fam[1], fam[2]
    sing = (np.zeros(6, np.int32), np.array([1, 1, 1, 2, 2, 2], np.float32), np.ones(6, np.float32))
    pts3 = [pts[0], sing, pts[1]]
    th3 = np.stack([th[0], th[0], th[1]])
    th3[1, :D] = -80.0   # no noise: the reference's jitter loop gives up (status -1)
    bad = CC.points(5, D, sing[1], 40)
    ctx = make_ctx(*fam, pts3)
    out, st = ctx.components([0, 1, 2], th3, [qs[0][0], bad[0], qs[1][0]], [qs[0][1], bad[1], qs[1][1]])
    ctx.close()
    assert st[1] < 0 and st[0] == 0 and st[2] == 0
    assert out[1][0].shape == (40, Q) and out[1][2].shape == (40, Q, Q) and all(np.all(np.isnan(a)) for a in out[1])
    for i, p in ((0, 0), (2, 1)):
        CR.check_components(Q, CR.restate(*CC.fam_args(fam, pts[p]), th[p], qs[p][0], qs[p][1]), out[i])   # (no jitter here)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b, what, n=3):
    for k in range(n):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, CR.NAMES[k])


def test_point_outputs_are_bit_invariant(monkeypatch):
    fam, pts, th, qs = CC.case_data("bits")
    m2s, t2s = CC.call_lists(fam, qs)
    ctx = make_ctx(*fam, pts)
    ctx.pin_route(True)
    ref, st = ctx.components([0, 1], th, m2s, t2s)
    assert np.all(st == 0)
    check_case("bits", fam, ref)
    # without ccov: the other two unchanged
    noc, _ = ctx.components([0, 1], th, m2s, t2s, cov=False)
    for p in range(2):
        assert noc[p][2] is None
        _same(noc[p], ref[p], ("cov=False", p), 2)
    # shuffled positions: other tiles, other columns, other pair threads
    perm = [np.random.default_rng(1).permutation(len(m2s[p])) for p in range(2)]
    sh, _ = ctx.components([0, 1], th, [m2s[p][perm[p]] for p in range(2)], [t2s[p][perm[p]] for p in range(2)])
    for p in range(2):
        _same(sh[p], [a[perm[p]] for a in ref[p]], ("shuffled", p))
    # a point alone
    e0, e1 = np.zeros(0, np.int32), np.zeros(0, np.float32)
    for p, j in ((0, 0), (0, 77), (1, 149), (1, 32)):
        one, _ = ctx.components([0, 1], th, [m2s[q][j:j + 1] if q == p else e0 for q in range(2)], [t2s[q][j:j + 1] if q == p else e1 for q in range(2)])
        _same(one[p], [a[j:j + 1] for a in ref[p]], ("alone", p, j))
    # the call split in two (route pinned: the patients lose their batch-mate)
    for p in range(2):
        half, _ = ctx.components([p], th[p:p + 1], [m2s[p]], [t2s[p]])
        _same(half[0], ref[p], ("split", p))
    ctx.close()
    # a work budget of one tile per launch chunk; the launches are accounted under the profile entry of k_posterior
    monkeypatch.setenv("MEDGP_POSTERIOR_BUDGET_GB", "1e-6")
    ctx = make_ctx(*fam, pts)
    ctx.pin_route(True)
    ctx.profile_enable(True, only="k_posterior")
    ch, _ = ctx.components([0, 1], th, m2s, t2s)
    launches = ctx.profile_read()["k_posterior"][1]
    ctx.close()
    P = 64 // fam[1]
    assert launches == sum(-(-len(x) // P) for x in t2s) == 5 + 8   # one per tile of 21 points (100 and 150 points)
    for p in range(2):
        _same(ch[p], ref[p], ("chunks", p))


def test_far_field():
    """t* = t_max + 5000 h (and t_min - 5000 h): the posterior of every component is its prior, exactly"""
    fam, pt, th, (m2, t2), prior = CC.far_case()
    Q = fam[1]
    ctx = make_ctx(*fam, [pt])
    out, st = ctx.components([0], th[None, :], [m2], [t2])
    ctx.close()
    cmean, cvar, ccov = out[0]
    assert st[0] == 0
    assert np.all(cmean == 0.0) and np.all(ccov[:, ~np.eye(Q, dtype=bool)] == 0.0)
    assert np.array_equal(cvar, prior.astype(np.float32)), (cvar, prior)
    assert np.array_equal(ccov[:, np.arange(Q), np.arange(Q)], cvar)


def test_argument_errors():
    """cmean or cvar NULL, bad offsets and Q = 65: MEDGP_ERR_ARG before any device work"""
    fam, pts, th, qs = CC.case_data("jitter")
    Q = fam[1]
    ctx = make_ctx(*fam, pts[:1])
    lib, h = ctx._lib, ctx._h
    i32, f32 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_float)))
    m2, t2 = qs[0]
    M = t2.shape[0]
    slots, st = np.zeros(1, np.int32), np.zeros(1, np.int32)
    theta = np.ascontiguousarray(th[0])
    o = [np.full(M * Q, 7.0, np.float32), np.full(M * Q, 7.0, np.float32), np.full(M * Q * Q, 7.0, np.float32)]

    def call(off, drop=()):
        off = np.asarray(off, np.int64)
        a = [h, 1, i32(slots), theta.ctypes.data_as(C.POINTER(C.c_double)), off.ctypes.data_as(C.POINTER(C.c_int64)), i32(m2), f32(t2)] \
            + [f32(x) for x in o] + [i32(st)]
        for k in drop:
            a[k] = None
        return lib.medgp_components_batch(*a)
    ctx.profile_enable(True)
    assert call([0, M], (7,)) == -1 and call([0, M], (8,)) == -1 and call([0, M], (7, 8)) == -1
    assert call([1, M]) == -1 and call([0, -1]) == -1
    assert all(n == 0 for _, n in ctx.profile_read().values())     # nothing was launched
    assert all(np.all(x == 7.0) for x in o)                        # and nothing written
    assert call([0, M], (9,)) == 0                                 # ccov may be NULL
    assert np.all(o[2] == 7.0) and not np.any(o[0] == 7.0) and not np.any(o[1] == 7.0)
    ctx.close()
    # Q = 65: a point's columns do not fit one tile
    D, R = 2, 1
    pt = synth.patient(3, 0, D, 20)
    ctx = make_ctx(7, 65, D, R, [pt])
    ctx.profile_enable(True)
    with pytest.raises(medgp_amd.MedgpError, match="Q <= 64"):
        ctx.components([0], np.zeros((1, ctx.H)), [np.zeros(2, np.int32)], [np.zeros(2, np.float32)])
    assert all(n == 0 for _, n in ctx.profile_read().values())
    ctx.close()
