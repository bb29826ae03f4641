"""medgp_functional_batch on the MI355X: parity with the numpy definition (functional_ref.py) on the inputs of functional_cases.py --
the three covariance families, Q <= 8 and Q = 17, n under, on and over the 64-row panel, functional counts on and around the 64-column
tile, term counts 0, 1, 2, 25 and 70 inside one tile with zero and negative weights, every factorisation route -- the contrast of a
point with itself, consistency of single-term functionals with medgp_posterior_batch, jitter rounds and failed entries, the bits of a
functional's outputs (unchanged by the functionals' order, the split of a call and the launch chunks), the far field and the argument
errors.  Every parity test prints its worst error per quantity in fp32 ulps (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
from medgp_amd import functionals as FN
import functional_cases as FC
import functional_ref as FR
import posterior_ref as PR


def make_ctx(kidx, Q, D, R, pts):
    ctx = medgp_amd.Context(kidx, Q, D, R)
    ctx.reserve(len(pts), max(max(p[1].shape[0] for p in pts), 1), len(pts))
    for s, (m, t, y) in enumerate(pts):
        ctx.set_patient(s, m if kidx == 7 else None, t, y)
    return ctx


def check_case(name, out, sel=None, who=""):
    """out[i] of patient sel[i] against the shared reference; prints the worst error per quantity"""
    sel = FC.checked(name) if sel is None else sel
    worst = [0.0] * 2
    for i, p in enumerate(sel):
        u = FR.check_functional(FC.case_ref(name, p), out[i])
        worst = [max(a, b) for a, b in zip(worst, u)]
    print(f"{name}{who}: " + " ".join(f"{n} {x:.3f}" for n, x in zip(FR.NAMES, worst)) + " (fp32 ulps)")


def check_single_terms(fam, ctx, pts, th, qs, out):
    """the single-term functionals of weight 1 of every patient against medgp_posterior_batch at the same points, with the rule of
    check_sums (test_components_gpu.py): |fmean - mean| <= 4e-7 (|fmean| + |mean|), |fvar + sigma^2 - var| <= 4e-7 (|fvar + sigma^2| + |var|)"""
    kidx, _, D, _ = fam
    idx, m2s, t2s = [], [], []
    for p in range(len(pts)):
        toff, m2, t2, a = qs[p]
        one = np.array([f for f in range(len(toff) - 1) if toff[f + 1] - toff[f] == 1 and a[toff[f]] == 1.0], np.int64)
        idx.append(one)
        m2s.append(m2[toff[one]])
        t2s.append(t2[toff[one]])
    assert sum(len(i) for i in idx) > 0
    post, pst = ctx.posterior(np.arange(len(pts)), th, m2s if kidx == 7 else None, t2s, parts=False)
    for p in range(len(pts)):
        fmean, fvar = (x[idx[p]].astype(np.float64) for x in out[p])
        mean, var = post[p][0].astype(np.float64), post[p][1].astype(np.float64)
        lat = fvar + PR.noise_var(kidx, D, th[p], m2s[p] if kidx == 7 else np.zeros(len(idx[p]), np.int32))
        assert np.all(np.abs(fmean - mean) <= 4e-7 * (np.abs(fmean) + np.abs(mean))), ("mean", p)
        assert np.all(np.abs(lat - var) <= 4e-7 * (np.abs(lat) + np.abs(var))), ("var", p)


def run_case(name, with_posterior=False):
    fam, pts, th, qs = FC.case_data(name)
    ctx = make_ctx(*fam, pts)
    out, st = ctx.functionals(np.arange(len(pts)), th, FC.call_list(qs))
    plan = ctx.last_plan()
    if with_posterior:
        check_single_terms(fam, ctx, pts, th, qs, out)
    ctx.close()
    return fam, pts, th, qs, out, st, plan


@pytest.mark.parametrize("name", ["parity_d3", "parity_d24", "q17", "se", "sm"])
def test_parity_with_definition_and_single_terms_with_posterior(name):
    fam, pts, th, qs, out, st, _ = run_case(name, True)   # (parity_d3 / parity_d24: interleaved upload, the callers' order, not grouped)
    assert np.all(st == 0)
    check_case(name, out)


def test_tile_edges():
    fam, pts, th, qs, out, st, _ = run_case("tile_edges")
    assert np.all(st == 0)
    for p, k in enumerate(FC.EDGE_COUNTS):
        assert out[p][0].shape == (k,) and out[p][1].shape == (k,)
    check_case("tile_edges", out)


def test_term_counts_in_one_tile_and_degenerate_contrast():
    """36 + 3 functionals in one tile: 0, 1, 2, 25 and 70 terms, zero and negative weights; a functional without terms gives exactly
    0.0f / 0.0f; the contrast of a point with itself stays within the bar of 0 (the reference is exactly 0; exact zero not required)"""
    fam, pts, th, qs, out, st, _ = run_case("degenerate")
    toff, m2, t2, a = qs[0]
    cnt = np.diff(toff)
    assert len(cnt) <= 64 and set(cnt.tolist()) == {0, 1, 2, 25, 70} and np.any(a == 0.0) and np.any(a < 0.0)
    assert st[0] == 0
    for k in range(2):
        assert not np.any(out[0][k][cnt == 0].view(np.uint32)), "a functional without terms must give +0.0f"
    check_case("degenerate", out)
    ref = FC.case_ref("degenerate", 0)
    for k in range(2):
        bar = 2.0 ** -22 * 1e-3 * np.abs(ref[k]).max()
        assert np.all(ref[k][-FC.N_DEGENERATE:] == 0.0) and np.all(np.abs(out[0][k][-FC.N_DEGENERATE:]) <= bar)


def test_routes_all_three_and_pinned():
    """One call whose size classes take the 4-wave (route 0), 8-wave (1) and look-ahead (2) factorisations."""
    fam, pts, th, qs = FC.case_data("routes")
    chk = FC.ROUTE_CHECKED
    ctx = make_ctx(*fam, pts)
    out, st = ctx.functionals(np.arange(len(pts)), th, FC.call_list(qs))
    assert {r for (_, _, r) in ctx.last_plan()} == {0, 1, 2}, ctx.last_plan()
    assert np.all(st == 0)
    assert all(out[p][0].shape == (0,) for p in range(len(pts)) if p not in chk)
    check_case("routes", [out[p] for p in chk], chk)
    ctx.pin_route(True)
    out2, st2 = ctx.functionals(chk, th[chk], FC.call_list(qs, chk))
    assert {r for (_, _, r) in ctx.last_plan()} == {1}
    assert np.all(st2 == 0)
    check_case("routes", out2, chk, " pinned")
    ctx.close()


def test_forced_multi_cu_route(monkeypatch):
    monkeypatch.setenv("MEDGP_MULTI_CU", "1")
    fam, pts, th, qs, out, st, plan = run_case("multi_cu")
    assert {r for (_, _, r) in plan} == {2}
    assert np.all(st == 0)
    check_case("multi_cu", out)


def test_jitter_rounds(monkeypatch):
    """MEDGP_DEBUG_FAIL_ATTEMPTS = 2: every quantity is that of the factor of K + 2 diag(sigma^2) (restate(jitter_rounds = 2))"""
    monkeypatch.setenv("MEDGP_DEBUG_FAIL_ATTEMPTS", str(FC.JITTER_ROUNDS["jitter"]))
    fam, pts, th, qs, out, st, _ = run_case("jitter")
    assert np.all(st == FC.JITTER_ROUNDS["jitter"]), st
    check_case("jitter", out)


def test_failed_entry_gives_nan_and_spares_batch_mates():
    fam, pts, th, qs = FC.case_data("jitter")
    D = fam[2]
    sing = (np.zeros(6, np.int32), np.array([1, 1, 1, 2, 2, 2], np.float32), np.ones(6, np.float32))
    pts3 = [pts[0], sing, pts[1]]
    th3 = np.stack([th[0], th[0], th[1]])
    th3[1, :D] = -80.0   # no noise: the reference's jitter loop gives up (status -1)
    bad = FN.pack(FC.mix(5, D, sing[1], 40))
    ctx = make_ctx(*fam, pts3)
    out, st = ctx.functionals([0, 1, 2], th3, [qs[0], bad, qs[1]])
    ctx.close()
    assert st[1] < 0 and st[0] == 0 and st[2] == 0
    assert out[1][0].shape == (40,) and all(np.all(np.isnan(a)) for a in out[1])
    for i, p in ((0, 0), (2, 1)):
        FR.check_functional(FC.restate(fam, pts[p], th[p], qs[p]), out[i])   # (no jitter here)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b, what):
    for k in range(2):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, FR.NAMES[k])


def test_functional_outputs_are_bit_invariant(monkeypatch):
    fam, pts, th, _ = FC.case_data("bits")
    lists = FC.case_lists("bits")
    packed = [FN.pack(fs) for fs in lists]
    ctx = make_ctx(*fam, pts)
    ctx.pin_route(True)
    ref, st = ctx.functionals([0, 1], th, packed)
    assert np.all(st == 0)
    check_case("bits", ref)
    # shuffled positions: other tiles, other columns, other neighbours in the wave
    perm = [np.random.default_rng(1).permutation(len(lists[p])) for p in range(2)]
    sh, _ = ctx.functionals([0, 1], th, [FN.pack([lists[p][j] for j in perm[p]]) for p in range(2)])
    for p in range(2):
        _same(sh[p], [a[perm[p]] for a in ref[p]], ("shuffled", p))
    # a functional alone (a point, a 24 h mean, 70 random terms, a 0.25 h change)
    for p, j in ((0, 0), (0, 1), (1, 75), (1, 3)):
        one, _ = ctx.functionals([0, 1], th, [FN.pack([lists[q][j]] if q == p else []) for q in range(2)])
        assert one[1 - p][0].shape == (0,)
        _same(one[p], [a[j:j + 1] for a in ref[p]], ("alone", p, j))
    # the call split per patient (route pinned: the patients lose their batch-mate)
    for p in range(2):
        half, _ = ctx.functionals([p], th[p:p + 1], [packed[p]])
        _same(half[0], ref[p], ("split", p))
    ctx.close()
    # a work budget of one tile per launch chunk; the launches are accounted under the profile entry of k_posterior
    monkeypatch.setenv("MEDGP_POSTERIOR_BUDGET_GB", "1e-6")
    ctx = make_ctx(*fam, pts)
    ctx.pin_route(True)
    ctx.profile_enable(True, only="k_posterior")
    ch, _ = ctx.functionals([0, 1], th, packed)
    launches = ctx.profile_read()["k_posterior"][1]
    ctx.close()
    assert launches == sum(-(-len(x) // 64) for x in lists) == 2 + 2   # one per tile of 64 functionals (70 and 100 functionals)
    for p in range(2):
        _same(ch[p], ref[p], ("chunks", p))


def test_far_field():
    """every term at t_max + 5000 h or t_min - 5000 h: fmean is exactly 0 and fvar the prior's q_g, rounded once"""
    fam, pt, th, packed, qg = FC.far_case()
    ctx = make_ctx(*fam, [pt])
    out, st = ctx.functionals([0], th[None, :], [packed])
    ctx.close()
    assert st[0] == 0
    assert np.all(out[0][0] == 0.0)
    FR.check_functional((np.zeros_like(qg), qg, qg), out[0])
    assert np.all(np.abs(out[0][1].astype(np.float64) - qg) <= 2.0 ** -23 * qg)


def test_argument_errors():
    """NULL outputs, NULL weight / t2 / toffsets / foffsets, NULL meta2 on LMC-SM and broken offsets: MEDGP_ERR_ARG before any device
    work -- the profile counters stay at zero and the output buffers untouched"""
    fam, pts, th, qs = FC.case_data("jitter")
    ctx = make_ctx(*fam, pts[:1])
    lib, h = ctx._lib, ctx._h
    i32, i64, f32, f64 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))), \
        (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    toff, m2, t2, a = qs[0]
    F = toff.shape[0] - 1
    slots, st = np.zeros(1, np.int32), np.zeros(1, np.int32)
    theta = np.ascontiguousarray(th[0])
    o = [np.full(F, 7.0, np.float32), np.full(F, 7.0, np.float32)]

    def call(foff=(0, F), toffs=toff, drop=()):
        foff, toffs = np.asarray(foff, np.int64), np.ascontiguousarray(toffs, np.int64)
        args = [h, 1, i32(slots), f64(theta), i64(foff), i64(toffs), i32(m2), f32(t2), f64(a), f32(o[0]), f32(o[1]), i32(st)]
        for k in drop:
            args[k] = None
        return lib.medgp_functional_batch(*args)
    ctx.profile_enable(True)
    for k in (4, 5, 6, 7, 8, 9, 10):
        assert call(drop=(k,)) == -1, k
    assert call(drop=(9, 10)) == -1
    assert call(foff=(1, F)) == -1 and call(foff=(0, -1)) == -1
    bad = toff.copy()
    bad[0] = 1
    assert call(toffs=bad) == -1
    bad = toff.copy()
    bad[F // 2] = bad[F // 2 + 1] + 1
    assert call(toffs=bad) == -1
    bad = toff.copy()
    bad[-1] = 2 ** 31
    assert call(toffs=bad) == -1
    assert all(n == 0 for _, n in ctx.profile_read().values())     # nothing was launched
    assert all(np.all(x == 7.0) for x in o)                        # and nothing written
    assert call() == 0
    assert not np.any(o[0][np.diff(toff) > 0] == 7.0) and not np.any(o[1] == 7.0)
    ctx.close()
