"""medgp_trend_batch on the MI355X: parity with the numpy definition (trend_ref.py) on the inputs of trend_cases.py -- the three
covariance families, the table (Q <= 8) and the generic (Q = 17) component loops, every factorisation route, point counts on and
around the 32-point tile edge -- jitter rounds and failed entries, the bits of a point's outputs (equal to medgp_posterior_batch's
mean / var; unchanged by the points' order, the split of a call and the launch chunks), the far field and the argument errors.
Every parity test prints its worst error per quantity in fp32 ulps (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
from medgp_amd import synth
import trend_cases as TC
import trend_ref as TR


def make_ctx(kidx, Q, D, R, pts):
    ctx = medgp_amd.Context(kidx, Q, D, R)
    ctx.reserve(len(pts), max(max(p[1].shape[0] for p in pts), 1), len(pts))
    for s, (m, t, y) in enumerate(pts):
        ctx.set_patient(s, m if kidx == 7 else None, t, y)
    return ctx


def check_case(name, fam, th, qs, out, sel=None, who=""):
    """out[i] of patient sel[i] against the shared reference; prints the worst error per quantity"""
    sel = TC.checked(name) if sel is None else sel
    worst = [0.0] * 5
    for i, p in enumerate(sel):
        m2 = qs[p][0] if fam[0] == 7 else None
        u = TR.check_trend(fam[0], fam[2], th[p], m2, TC.case_ref(name, p), out[i])
        worst = [max(a, b) for a, b in zip(worst, u)]
    print(f"{name}{who}: " + " ".join(f"{n} {x:.3f}" for n, x in zip(TR.NAMES, worst)) + " (fp32 ulps)")


def run_case(name):
    fam, pts, th, qs = TC.case_data(name)
    ctx = make_ctx(*fam, pts)
    m2s, t2s = TC.call_lists(fam, qs)
    out, st = ctx.trend(np.arange(len(pts)), th, m2s, t2s)
    plan = ctx.last_plan()
    ctx.close()
    return fam, pts, th, qs, out, st, plan


@pytest.mark.parametrize("name", ["parity_d3", "parity_d24"])
def test_parity_with_definition(name):
    fam, pts, th, qs, out, st, _ = run_case(name)   # interleaved upload: the callers' order, not grouped
    assert np.all(st == 0)
    check_case(name, fam, th, qs, out)


def test_tile_edges():
    fam, pts, th, qs, out, st, _ = run_case("tile_edges")
    assert np.all(st == 0)
    for p, k in enumerate(TC.EDGE_COUNTS):
        assert all(a.shape == (k,) for a in out[p])
    check_case("tile_edges", fam, th, qs, out)


@pytest.mark.parametrize("name", ["generic_q17", "se", "sm"])
def test_generic_route_and_single_output_families(name):
    fam, pts, th, qs, out, st, _ = run_case(name)   # (se / sm: meta2 = None)
    assert np.all(st == 0)
    check_case(name, fam, th, qs, out)


def test_routes_all_three_and_pinned():
    """One call whose size classes take the 4-wave (route 0), 8-wave (1) and look-ahead (2) factorisations."""
    fam, pts, th, qs = TC.case_data("routes")
    chk = TC.ROUTE_CHECKED
    ctx = make_ctx(*fam, pts)
    m2s, t2s = TC.call_lists(fam, qs)
    out, st = ctx.trend(np.arange(len(pts)), th, m2s, t2s)
    assert {r for (_, _, r) in ctx.last_plan()} == {0, 1, 2}, ctx.last_plan()
    assert np.all(st == 0)
    assert all(out[p][0].shape == (0,) for p in range(len(pts)) if p not in chk)
    check_case("routes", fam, th, qs, [out[p] for p in chk], chk)
    ctx.pin_route(True)
    m2c, t2c = TC.call_lists(fam, qs, chk)
    out2, st2 = ctx.trend(chk, th[chk], m2c, t2c)
    assert {r for (_, _, r) in ctx.last_plan()} == {1}
    assert np.all(st2 == 0)
    check_case("routes", fam, th, qs, out2, chk, " pinned")
    ctx.close()


def test_forced_multi_cu_route(monkeypatch):
    monkeypatch.setenv("MEDGP_MULTI_CU", "1")
    fam, pts, th, qs, out, st, plan = run_case("multi_cu")
    assert {r for (_, _, r) in plan} == {2}
    assert np.all(st == 0)
    check_case("multi_cu", fam, th, qs, out)


def test_jitter_rounds(monkeypatch):
    """MEDGP_DEBUG_FAIL_ATTEMPTS = 2: every quantity is that of the factor of K + 2 diag(sigma^2) (restate(jitter_rounds = 2))"""
    monkeypatch.setenv("MEDGP_DEBUG_FAIL_ATTEMPTS", str(TC.JITTER_ROUNDS["jitter"]))
    fam, pts, th, qs, out, st, _ = run_case("jitter")
    assert np.all(st == TC.JITTER_ROUNDS["jitter"]), st
    check_case("jitter", fam, th, qs, out)


def test_failed_entry_gives_nan_and_spares_batch_mates():
    fam, pts, th, qs = TC.case_data("jitter")
    D = fam[2]
    sing = (np.zeros(6, np.int32), np.array([1, 1, 1, 2, 2, 2], np.float32), np.ones(6, np.float32))
    pts3 = [pts[0], sing, pts[1]]
    th3 = np.stack([th[0], th[0], th[1]])
    th3[1, :D] = -80.0   # no noise: the reference's jitter loop gives up (status -1)
    bad = TC.points(5, D, sing[1], 40)
    ctx = make_ctx(*fam, pts3)
    out, st = ctx.trend([0, 1, 2], th3, [qs[0][0], bad[0], qs[1][0]], [qs[0][1], bad[1], qs[1][1]])
    ctx.close()
    assert st[1] < 0 and st[0] == 0 and st[2] == 0
    assert all(a.shape == (40,) and np.all(np.isnan(a)) for a in out[1])
    for i, p in ((0, 0), (2, 1)):
        TR.check_trend(fam[0], D, th[p], qs[p][0], TR.restate(*TC.fam_args(fam, pts[p]), th[p], qs[p][0], qs[p][1]), out[i])   # (no jitter here)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b, what):
    for k in range(5):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, TR.NAMES[k])


def test_point_outputs_are_bit_invariant(monkeypatch):
    fam, pts, th, qs = TC.case_data("bits")
    m2s, t2s = TC.call_lists(fam, qs)
    ctx = make_ctx(*fam, pts)
    ctx.pin_route(True)
    ref, st = ctx.trend([0, 1], th, m2s, t2s)
    assert np.all(st == 0)
    check_case("bits", fam, th, qs, ref)
    # mean and var are medgp_posterior_batch's, bit for bit
    post, _ = ctx.posterior([0, 1], th, m2s, t2s, parts=False)
    for p in range(2):
        assert np.array_equal(_bits(post[p][0]), _bits(ref[p][0])), ("mean", p)
        assert np.array_equal(_bits(post[p][1]), _bits(ref[p][1])), ("var", p)
    # without cross: the other four unchanged
    noc, _ = ctx.trend([0, 1], th, m2s, t2s, cross=False)
    for p in range(2):
        assert noc[p][4] is None
        for k in range(4):
            assert np.array_equal(_bits(noc[p][k]), _bits(ref[p][k])), (p, k)
    # shuffled positions: other tiles, other columns
    perm = [np.random.default_rng(1).permutation(len(m2s[p])) for p in range(2)]
    sh, _ = ctx.trend([0, 1], th, [m2s[p][perm[p]] for p in range(2)], [t2s[p][perm[p]] for p in range(2)])
    for p in range(2):
        _same(sh[p], [a[perm[p]] for a in ref[p]], ("shuffled", p))
    # a point alone
    e0, e1 = np.zeros(0, np.int32), np.zeros(0, np.float32)
    for p, j in ((0, 0), (0, 77), (1, 149), (1, 32)):
        one, _ = ctx.trend([0, 1], th, [m2s[q][j:j + 1] if q == p else e0 for q in range(2)], [t2s[q][j:j + 1] if q == p else e1 for q in range(2)])
        _same(one[p], [a[j:j + 1] for a in ref[p]], ("alone", p, j))
    # the call split in two (route pinned: the patients lose their batch-mate)
    for p in range(2):
        half, _ = ctx.trend([p], th[p:p + 1], [m2s[p]], [t2s[p]])
        _same(half[0], ref[p], ("split", p))
    ctx.close()
    # a work budget of one tile per launch chunk
    monkeypatch.setenv("MEDGP_POSTERIOR_BUDGET_GB", "1e-6")
    ctx = make_ctx(*fam, pts)
    ctx.pin_route(True)
    ctx.profile_enable(True, only="k_trend")
    ch, _ = ctx.trend([0, 1], th, m2s, t2s)
    launches = ctx.profile_read()["k_trend"][1]
    ctx.close()
    assert launches == 4 + 5   # one per tile of 32 points (100 and 150 points)
    for p in range(2):
        _same(ch[p], ref[p], ("chunks", p))


def test_far_field():
    """t* = t_max + 5000 h (and t_min - 5000 h): the slope's posterior is its prior, exactly"""
    fam, pt, th, (m2, t2), prior = TC.far_case()
    ctx = make_ctx(*fam, [pt])
    out, st = ctx.trend([0], th[None, :], [m2], [t2])
    ctx.close()
    mean, var, dmean, dvar, cross = out[0]
    assert st[0] == 0
    assert np.all(dmean == 0.0) and np.all(cross == 0.0) and np.all(mean == 0.0)
    assert np.array_equal(dvar, prior.astype(np.float32)), (dvar, prior)


def test_argument_errors():
    """dmean or dvar NULL and bad offsets: MEDGP_ERR_ARG before any device work"""
    fam, pts, th, qs = TC.case_data("jitter")
    ctx = make_ctx(*fam, pts[:1])
    lib, h = ctx._lib, ctx._h
    i32, f32 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_float)))
    m2, t2 = qs[0]
    M = t2.shape[0]
    slots, st = np.zeros(1, np.int32), np.zeros(1, np.int32)
    theta = np.ascontiguousarray(th[0])
    o = [np.full(M, 7.0, np.float32) for _ in range(5)]

    def call(off, drop=()):
        off = np.asarray(off, np.int64)
        a = [h, 1, i32(slots), theta.ctypes.data_as(C.POINTER(C.c_double)), off.ctypes.data_as(C.POINTER(C.c_int64)), i32(m2), f32(t2)] \
            + [f32(x) for x in o] + [i32(st)]
        for k in drop:
            a[k] = None
        return lib.medgp_trend_batch(*a)
    ctx.profile_enable(True)
    assert call([0, M], (9,)) == -1 and call([0, M], (10,)) == -1 and call([0, M], (9, 10)) == -1
    assert call([1, M]) == -1 and call([0, -1]) == -1
    assert all(n == 0 for _, n in ctx.profile_read().values())     # nothing was launched
    assert all(np.all(x == 7.0) for x in o)                        # and nothing written
    assert call([0, M], (11,)) == 0                                # cross may be NULL
    assert np.all(o[4] == 7.0) and not np.any(o[2] == 7.0)
    ctx.close()
