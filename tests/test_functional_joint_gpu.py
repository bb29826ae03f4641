"""medgp_functional_joint_batch on the MI355X: parity of fmean, fvar and fcov with the numpy definition (functional_joint_ref.py) on the
inputs of functional_cases.py -- n in {5, 70, 131, 200, 300, ...}, functional counts 0, 1, 63, 64, 65 and 130 (one, two and three
tiles: diagonal and off-diagonal tile pairs), 0 to 70 terms inside one tile, the three covariance families, Q <= 8 and Q = 17, every
factorisation route, jitter rounds; fmean / fvar bit-identical to medgp_functional_batch; fcov exactly symmetric with the bits of fvar
on its diagonal and exact zeros for empty functionals; the bits of a pair's covariance unchanged by a subset of the functionals, the
split of a call and the launch chunks; a failed entry; consistency with medgp_posterior_joint_batch; the capacity and argument errors.
Every parity test prints its worst error per quantity in fp32 ulps (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
from medgp_amd import functionals as FN
import functional_cases as FC
import functional_joint_ref as FJ
import posterior_ref as PR


def make_ctx(kidx, Q, D, R, pts):
    ctx = medgp_amd.Context(kidx, Q, D, R)
    ctx.reserve(len(pts), max(max(p[1].shape[0] for p in pts), 1), len(pts))
    for s, (m, t, y) in enumerate(pts):
        ctx.set_patient(s, m if kidx == 7 else None, t, y)
    return ctx


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_structure(packed, out):
    """what holds without a reference: shapes, exact symmetry, the diagonal, the rows and columns of the functionals without terms"""
    F = packed[0].shape[0] - 1
    fmean, fvar, fcov = out
    assert fmean.shape == (F,) and fvar.shape == (F,) and fcov.shape == (F, F) and fcov.dtype == np.float32
    b = _bits(fcov)
    assert np.array_equal(b, b.T), "fcov is not exactly symmetric"
    assert np.array_equal(np.diag(b), _bits(fvar)), "the diagonal of fcov does not have the bits of fvar"
    empty = np.diff(packed[0]) == 0
    assert not np.any(b[empty]) and not np.any(b[:, empty]), "a functional without terms must give a row and a column of +0.0f"


def check_case(name, out, sel=None, who=""):
    """out[i] of patient sel[i] against the shared reference; prints the worst error per quantity"""
    sel = FC.checked(name) if sel is None else sel
    qs = FC.case_data(name)[3]
    worst = [0.0] * 3
    for i, p in enumerate(sel):
        check_structure(qs[p], out[i])
        u = FJ.check_joint(FJ.case_ref(name, p), out[i])
        worst = [max(a, b) for a, b in zip(worst, u)]
    print(f"{name}{who}: " + " ".join(f"{n} {x:.3f}" for n, x in zip(FJ.NAMES, worst)) + " (fp32 ulps)")


def same_as_functionals(ctx, slots, th, plist, out):
    """fmean / fvar of the joint call are medgp_functional_batch's on the same call, bit for bit"""
    ref, _ = ctx.functionals(slots, th, plist)
    for p in range(len(plist)):
        for k in range(2):
            assert np.array_equal(_bits(out[p][k]), _bits(ref[p][k])) and out[p][k].shape == ref[p][k].shape, (p, FJ.NAMES[k])


def run_case(name):
    fam, pts, th, qs = FC.case_data(name)
    ctx = make_ctx(*fam, pts)
    slots, plist = np.arange(len(pts)), FC.call_list(qs)
    out, st = ctx.functionals_joint(slots, th, plist)
    plan = ctx.last_plan()
    same_as_functionals(ctx, slots, th, plist, out)
    ctx.close()
    return fam, pts, th, qs, out, st, plan


@pytest.mark.parametrize("name", ["parity_d3", "parity_d24", "q17", "se", "sm"])
def test_parity_with_definition(name):
    fam, pts, th, qs, out, st, _ = run_case(name)
    assert np.all(st == 0)
    check_case(name, out)


def test_tile_edges():
    """F = 0, 1, 63, 64, 65 and 130 functionals of one patient: one, two and three tiles, diagonal and off-diagonal tile pairs"""
    fam, pts, th, qs, out, st, _ = run_case("tile_edges")
    assert np.all(st == 0)
    for p, k in enumerate(FC.EDGE_COUNTS):
        assert out[p][0].shape == (k,) and out[p][2].shape == (k, k)
    check_case("tile_edges", out)


def test_term_counts_in_one_tile_and_degenerate_contrast():
    """36 + 3 functionals in one tile with 0, 1, 2, 25 and 70 terms: the covariances of the contrast of a point with itself stay
    within the bar of 0 (the reference is exactly 0)"""
    fam, pts, th, qs, out, st, _ = run_case("degenerate")
    assert st[0] == 0 and set(np.diff(qs[0][0]).tolist()) == {0, 1, 2, 25, 70}
    check_case("degenerate", out)
    ref = FJ.case_ref("degenerate", 0)
    bar = 2.0 ** -22 * 1e-3 * np.abs(ref[2]).max()
    assert np.all(ref[2][-FC.N_DEGENERATE:] == 0.0) and np.all(np.abs(out[0][2][-FC.N_DEGENERATE:]) <= bar)


def test_routes_all_three_and_pinned():
    """One call whose size classes take the 4-wave (route 0), 8-wave (1) and look-ahead (2) factorisations."""
    fam, pts, th, qs = FC.case_data("routes")
    chk = FC.ROUTE_CHECKED
    ctx = make_ctx(*fam, pts)
    out, st = ctx.functionals_joint(np.arange(len(pts)), th, FC.call_list(qs))
    assert {r for (_, _, r) in ctx.last_plan()} == {0, 1, 2}, ctx.last_plan()
    assert np.all(st == 0)
    assert all(out[p][2].shape == (0, 0) for p in range(len(pts)) if p not in chk)
    check_case("routes", [out[p] for p in chk], chk)
    ctx.pin_route(True)
    out2, st2 = ctx.functionals_joint(chk, th[chk], FC.call_list(qs, chk))
    assert {r for (_, _, r) in ctx.last_plan()} == {1}
    assert np.all(st2 == 0)
    same_as_functionals(ctx, chk, th[chk], FC.call_list(qs, chk), out2)
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
    """a patient whose factorisation gives up (no noise, repeated observations: status -1) gets NaN in all three outputs; its
    neighbours' outputs are those of the call without it, bit for bit (route pinned)"""
    fam, pts, th, qs = FC.case_data("jitter")
    D = fam[2]
    sing = (np.zeros(6, np.int32), np.array([1, 1, 1, 2, 2, 2], np.float32), np.ones(6, np.float32))
    pts3 = [pts[0], sing, pts[1]]
    th3 = np.stack([th[0], th[0], th[1]])
    th3[1, :D] = -80.0
    bad = FN.pack(FC.mix(5, D, sing[1], 70))   # (two tiles: a diagonal and an off-diagonal pair of NaN)
    ctx = make_ctx(*fam, pts3)
    ctx.pin_route(True)
    out, st = ctx.functionals_joint([0, 1, 2], th3, [qs[0], bad, qs[1]])
    good, st2 = ctx.functionals_joint([0, 2], th3[[0, 2]], [qs[0], qs[1]])
    ctx.close()
    assert st[1] == -1 and st[0] == 0 and st[2] == 0 and np.all(st2 == 0)
    assert out[1][0].shape == (70,) and out[1][2].shape == (70, 70) and all(np.all(np.isnan(a)) for a in out[1])
    for i, j in ((0, 0), (2, 1)):
        for k in range(3):
            assert np.array_equal(_bits(out[i][k]), _bits(good[j][k])), (i, FJ.NAMES[k])
        FJ.check_joint(FJ.restate_case(fam, pts[j], th[j], qs[j]), out[i])   # (no jitter here)


def _sub(out, idx):
    return out[0][idx], out[1][idx], out[2][np.ix_(idx, idx)]


def _same(a, b, what):
    for k in range(3):
        assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), (what, FJ.NAMES[k])


def test_pair_covariances_are_bit_invariant(monkeypatch):
    """70 and 100 functionals (two tiles each): the covariance of a pair does not depend on the other functionals of the call and the
    tiles and columns the two land in (an order-preserving subset), on the batch-mate (each patient alone, route pinned) or on the
    launch chunks (a budget of one patient per chunk)."""
    fam, pts, th, _ = FC.case_data("bits")
    lists = FC.case_lists("bits")
    packed = [FN.pack(fs) for fs in lists]
    ctx = make_ctx(*fam, pts)
    ctx.pin_route(True)
    ctx.profile_enable(True, only="k_postcov")
    ref, st = ctx.functionals_joint([0, 1], th, packed)
    nclass = len(ctx.last_plan())
    blocks = max(b for (_, b, _) in ctx.last_plan())
    assert ctx.profile_read()["k_postcov"][1] == nclass   # one launch per chunk, one chunk per size class under the default budget
    ctx.profile_enable(False)
    assert np.all(st == 0)
    same_as_functionals(ctx, [0, 1], th, packed, ref)
    check_case("bits", ref)
    # an order-preserving subset: a pair keeps which of the two comes first, but lands in other tiles and columns
    g = np.random.default_rng(2)
    keep = [np.sort(g.choice(len(lists[p]), size=(len(lists[p]) * 3) // 5, replace=False)) for p in range(2)]
    assert [k.shape[0] for k in keep] == [42, 60] and all(k[0] < 64 <= k[-1] for k in keep)   # pairs of two tiles meet in one
    sub, _ = ctx.functionals_joint([0, 1], th, [FN.pack([lists[p][j] for j in keep[p]]) for p in range(2)])
    for p in range(2):
        _same(sub[p], _sub(ref[p], keep[p]), ("subset", p))
    # the last functionals alone: the second tile's diagonal pair becomes a first tile's
    tail = [np.arange(len(lists[p]) - 30, len(lists[p])) for p in range(2)]
    sub, _ = ctx.functionals_joint([0, 1], th, [FN.pack([lists[p][j] for j in tail[p]]) for p in range(2)])
    for p in range(2):
        _same(sub[p], _sub(ref[p], tail[p]), ("tail", p))
    # the call split per patient (route pinned: the patients lose their batch-mate)
    for p in range(2):
        half, _ = ctx.functionals_joint([p], th[p:p + 1], [packed[p]])
        _same(half[0], ref[p], ("split", p))
    ctx.close()
    # A budget that holds either patient but not both: one patient per launch chunk.  Bytes of a patient: its tiles' work rows
    # (ld x 64 doubles each, ld = 64 x the class's block count <= 64 x blocks) and F^2 floats.
    F = [len(x) for x in lists]
    n = [p[1].shape[0] for p in pts]
    hi = [-(-F[p] // 64) * 64 * blocks * 512 + 4 * F[p] ** 2 for p in range(2)]
    lo = [-(-F[p] // 64) * 64 * -(-n[p] // 64) * 512 + 4 * F[p] ** 2 for p in range(2)]
    budget = max(hi) + 1024
    assert sum(lo) > budget
    monkeypatch.setenv("MEDGP_POSTERIOR_BUDGET_GB", repr(budget / 2.0 ** 30))
    ctx = make_ctx(*fam, pts)
    ctx.pin_route(True)
    ctx.profile_enable(True)
    ch, st = ctx.functionals_joint([0, 1], th, packed)
    prof = ctx.profile_read()
    ctx.close()
    # one k_functional and one k_funccov launch per chunk = per patient; each k_funccov launch covers the patient's 3 lower tile pairs
    # (2 tiles: (0, 0), (1, 0), (1, 1)), 6 of the call
    pairs = [-(-f // 64) * (-(-f // 64) + 1) // 2 for f in F]
    assert pairs == [3, 3] and prof["k_postcov"][1] == 2 and prof["k_posterior"][1] == 2, prof
    assert np.all(st == 0)
    for p in range(2):
        _same(ch[p], ref[p], ("chunks", p))


def test_single_terms_against_the_joint_posterior():
    """Single-term functionals of weight 1 at 70 points of each patient (two tiles) against medgp_posterior_joint_batch (cov) at the
    same points: the off-diagonal elements agree within 4 fp32 ulps of max(|ref|, 1e-3 S), each side within 2 of the same reference
    (S: the largest |ref| of the latent block).  The diagonals differ by sigma^2 and are not compared in float."""
    fam, pts, th, _ = FC.case_data("parity_d3")
    D = fam[2]
    g = np.random.default_rng(9)
    m2s = [g.integers(0, D, size=70).astype(np.int32) for _ in pts]
    t2s = [g.uniform(float(p[1].min()) - 3.0, float(p[1].max()) + 3.0, size=70).astype(np.float32) for p in pts]
    plist = [FN.pack([FN.point(int(m), float(t)) for m, t in zip(m2s[p], t2s[p])]) for p in range(len(pts))]
    ctx = make_ctx(*fam, pts)
    slots = np.arange(len(pts))
    out, st = ctx.functionals_joint(slots, th, plist)
    post, pst, cst = ctx.posterior_joint(slots, th, m2s, t2s, None, cov=True)
    ctx.close()
    assert np.all(st == 0) and np.all(pst == 0) and np.all(cst == 0)
    worst = [0.0] * 3
    off = ~np.eye(70, dtype=bool)
    for p in range(len(pts)):
        ref = FJ.restate_case(fam, pts[p], th[p], plist[p])[2]
        scale = 2.0 ** -23 * np.maximum(np.abs(ref), 1e-3 * np.abs(ref).max())
        a, b = out[p][2].astype(np.float64), post[p][2].astype(np.float64)
        e = [float((np.abs(x)[off] / scale[off]).max()) for x in (a - ref, b - ref, a - b)]
        worst = [max(x, y) for x, y in zip(worst, e)]
        # the diagonal in fp64: fvar + sigma^2 is var up to the roundings of the two floats
        lat = np.diag(a) + PR.noise_var(fam[0], D, th[p], m2s[p])
        assert np.all(np.abs(lat - np.diag(b)) <= 4e-7 * (np.abs(lat) + np.abs(np.diag(b))))
    print(f"single terms: fcov {worst[0]:.3f} posterior_joint cov {worst[1]:.3f} between them {worst[2]:.3f} (fp32 ulps, off-diagonal)")
    assert worst[0] <= 2.0 and worst[1] <= 2.0 and worst[2] <= 4.0


def _raw(ctx, qs, th):
    """the raw library call on the one patient of ctx with prefilled outputs: call(foff, toffs, drop) -> return code"""
    lib, h = ctx._lib, ctx._h
    i32, i64, f32, f64 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))), \
        (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    toff, m2, t2, a = qs
    F = toff.shape[0] - 1
    slots, st = np.zeros(1, np.int32), np.zeros(1, np.int32)
    theta = np.ascontiguousarray(th)
    o = [np.full(F, 7.0, np.float32), np.full(F, 7.0, np.float32), np.full(F * F, 7.0, np.float32)]

    def call(foff=(0, F), toffs=toff, drop=()):
        foff, toffs = np.asarray(foff, np.int64), np.ascontiguousarray(toffs, np.int64)
        args = [h, 1, i32(slots), f64(theta), i64(foff), i64(toffs), i32(m2), f32(t2), f64(a), f32(o[0]), f32(o[1]), f32(o[2]), i32(st)]
        for k in drop:
            args[k] = None
        return lib.medgp_functional_joint_batch(*args)
    return call, o, toff, F


def test_single_patient_beyond_the_budget_is_a_capacity_error(monkeypatch):
    """1e-5 GB: the 40 functionals of one patient (n = 70: 32 KB of work rows and 6.4 KB of fcov) do not fit; MEDGP_ERR_CAPACITY with
    nothing launched behind the factorisation's set-up and nothing written; medgp_functional_batch on the same call still runs"""
    monkeypatch.setenv("MEDGP_POSTERIOR_BUDGET_GB", "1e-5")
    fam, pts, th, qs = FC.case_data("jitter")
    ctx = make_ctx(*fam, pts[:1])
    call, o, toff, F = _raw(ctx, qs[0], th[0])
    ctx.profile_enable(True)
    assert call() == -4   # MEDGP_ERR_CAPACITY
    msg = ctx._lib.medgp_last_error(ctx._h).decode()
    assert "MEDGP_POSTERIOR_BUDGET_GB" in msg and f"{F} functionals" in msg, msg
    assert all(n == 0 for _, n in ctx.profile_read().values())
    assert all(np.all(x == 7.0) for x in o)
    with pytest.raises(medgp_amd.MedgpError, match="MEDGP_POSTERIOR_BUDGET_GB"):
        ctx.functionals_joint([0], th[:1], [qs[0]])
    out, st = ctx.functionals([0], th[:1], [qs[0]])   # tile by tile
    assert st[0] == 0 and out[0][0].shape == (F,)
    ctx.close()


def test_argument_errors():
    """NULL outputs (fcov among them), NULL weight / t2 / toffsets / foffsets, NULL meta2 on LMC-SM and broken offsets: MEDGP_ERR_ARG
    before any device work -- the profile counters stay at zero and the output buffers untouched"""
    fam, pts, th, qs = FC.case_data("jitter")
    ctx = make_ctx(*fam, pts[:1])
    call, o, toff, F = _raw(ctx, qs[0], th[0])
    ctx.profile_enable(True)
    for k in (4, 5, 6, 7, 8, 9, 10, 11):
        assert call(drop=(k,)) == -1, k
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
    assert not np.any(o[1] == 7.0) and not np.any(o[2] == 7.0)
    check_structure(qs[0], (o[0], o[1], o[2].reshape(F, F)))
    ctx.close()
