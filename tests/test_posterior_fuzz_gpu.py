"""medgp_posterior_batch on seeded random shapes and at the corners the hand-picked cases of test_posterior_gpu.py do not reach:
D > 32 (per-covariate accumulators in the work rows), n = 1 / 2 and the 64-row panel boundaries, Q = 9 .. 16 and Q > 16 on the
generic k_posterior<0>, the generic assembly (MEDGP_V0) under the separable kernels, covariates the patient never observed, test
points on the training points, every factorisation route; then the jitter-retry path (MEDGP_DEBUG_FAIL_ATTEMPTS) on every output
that uses a factor, and the posterior interleaved with the other calls of a context.

Every float output is held to two fp32 ulps of the fp64 restatement (posterior_ref.check_posterior)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
from medgp_amd import synth
from oracle import oracle as O
from posterior_ref import assert_fp32_close, check_posterior, restate
from random_patients import random_patient

FORCED_N = (1, 2, 63, 64, 65, 128, 129)
NPTS = (0, 1, 63, 64, 65, 129, None)   # None: drawn
MODES = ("plain", "missing", "same_time", "shuffled", "burst")


def make_ctx(kidx, Q, D, R, pts):
    ctx = medgp_amd.Context(kidx, Q, D, R)
    ctx.reserve(len(pts), max(max(p[1].shape[0] for p in pts), 1), len(pts))
    for s, (m, t, y) in enumerate(pts):
        ctx.set_patient(s, m if kidx == 7 else None, t, y)
    return ctx


def sample_points(g, D, meta, t, k):
    """k test points: a third at random times over the data and 3 h beyond it, a third on training points (var cancels to
    near sigma^2 there), the rest on covariates the patient never observed (or random ones when it observed them all)"""
    if k == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.float32)
    unobs = np.setdiff1d(np.arange(D), meta)
    kind = g.integers(0, 3, size=k)
    m2 = g.integers(0, D, size=k).astype(np.int32)
    t2 = g.uniform(float(t.min()) - 3.0, float(t.max()) + 3.0, size=k).astype(np.float32)
    on = np.where(kind == 1)[0]
    src = g.integers(0, t.shape[0], size=on.size)
    m2[on], t2[on] = meta[src], t[src]
    if unobs.size:
        off = np.where(kind == 2)[0]
        m2[off] = g.choice(unobs, size=off.size)
    return m2, t2


CASES = []
_g = np.random.Generator(np.random.Philox(key=[20261016, 3]))
for c in range(16):
    D = int((1, 2, 3, 8, 24, 32, 33, 64)[c % 8])
    Q = int(_g.choice([1, 2, 3, 5, 8, 9, 12, 17]))
    R = int(_g.choice([1, 2, min(D, 4), D]))
    P = int(_g.integers(2, 5))
    ns = [FORCED_N[c % 7]] + [int(_g.integers(1, 331)) for _ in range(P - 1)]
    if c % 4 == 1:
        ns[-1] = 129 + int(_g.integers(0, 200))    # every fourth case has an entry for the look-ahead schedule
    npts = [int(_g.integers(2, 200)) if k is None else k for k in (NPTS[(c + p) % 7] for p in range(P))]
    CASES.append((c, D, Q, R, ns, npts, MODES[c % 5]))


def _case_id(c):
    return f"c{c[0]}_D{c[1]}Q{c[2]}R{c[3]}_{c[6]}_n{'-'.join(map(str, c[4]))}"


@functools.lru_cache(maxsize=None)
def _case_data(c):
    """(patients, theta, test points, references) of sweep case c (the references are shared by the routes)"""
    _, D, Q, R, ns, npts, mode = CASES[c]
    g = np.random.Generator(np.random.Philox(key=[5150, c]))
    pts = [random_patient(g, D, n, mode) for n in ns]
    th = np.stack([synth.theta(5150, 100 * c + p, 7, Q, D, R, sparse_frac=0.3 if c % 2 else 0.0) for p in range(len(ns))])
    tp = [sample_points(g, D, pts[p][0], pts[p][1], npts[p]) for p in range(len(ns))]
    refs = [restate(7, Q, D, R, pts[p][0], pts[p][1], pts[p][2], th[p], tp[p][0], tp[p][1]) for p in range(len(ns))]
    return pts, th, tp, refs


def _run_case(c, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _, D, Q, R, ns, _, _ = CASES[c]
    pts, th, tp, refs = _case_data(c)
    ctx = make_ctx(7, Q, D, R, pts)
    out, st = ctx.posterior(np.arange(len(ns)), th, [x[0] for x in tp], [x[1] for x in tp])
    plan = ctx.last_plan()
    ctx.close()
    assert np.all(st == 0), st
    for p in range(len(ns)):
        mean, var, parts = out[p]
        check_posterior(7, D, th[p], tp[p][0], refs[p], mean, var, parts)
        absent = np.setdiff1d(np.arange(D), pts[p][0])
        assert np.all(parts[:, absent].view(np.uint32) == 0), (p, absent)   # bit zero: no training row of that covariate
    return plan


ROUTED = [(case, route) for case in CASES for route in ("wg", "la", "auto") if route != "la" or max(case[4]) > 128]


@pytest.mark.parametrize("case,route", ROUTED, ids=lambda x: _case_id(x) if isinstance(x, tuple) else x)
def test_random_shapes_vs_restatement(case, route, monkeypatch):
    env = {"wg": {"MEDGP_MULTI_CU": "-1"}, "la": {"MEDGP_MULTI_CU": "1"}, "auto": {}}[route]
    monkeypatch.delenv("MEDGP_MULTI_CU", raising=False)
    plan = _run_case(case[0], monkeypatch, env)
    if route == "la":
        assert any(r == 2 for (_, _, r) in plan), plan


@pytest.mark.parametrize("c", [1, 2, 5, 7])
def test_random_shapes_generic_assembly(c, monkeypatch):
    """MEDGP_V0=1: the generic assembly k_assemble_v0 factors, the posterior still takes its separable k_posterior<Q <= 8>"""
    _run_case(c, monkeypatch, {"MEDGP_V0": "1"})


@pytest.mark.parametrize("kidx,Q", [(0, 1), (8, 1), (8, 3), (8, 8), (8, 9), (8, 12)])
def test_random_single_output_families(kidx, Q):
    g = np.random.Generator(np.random.Philox(key=[5151, 10 * kidx + Q]))
    ns = [1, 2, 65, int(g.integers(3, 330))]
    pts = []
    for n in ns:
        t = np.sort(g.uniform(0.0, 150.0, size=n)).astype(np.float32)
        pts.append((np.zeros(n, np.int32), t, g.standard_normal(n).astype(np.float32)))
    th = np.stack([synth.theta(5151, 10 * Q + p, kidx, Q, 1, 0) for p in range(len(ns))])
    tp = [sample_points(g, 1, *pts[p][:2], k)[1] for p, k in enumerate((5, 64, 129, 70))]
    ctx = make_ctx(kidx, Q, 1, 0, pts)
    out, st = ctx.posterior(np.arange(len(ns)), th, None, tp)
    ctx.close()
    assert np.all(st == 0)
    for p, (_, t, y) in enumerate(pts):
        ref = restate(kidx, Q, 1, 0, None, t, y, th[p], None, tp[p])
        check_posterior(kidx, 1, th[p], None, ref, *out[p])


def test_empty_patient_fails_alone():
    """n = 0: status -1 and NaN outputs (the header's status < 0), its batch-mates unaffected"""
    D, Q, R = 3, 3, 2
    g = np.random.Generator(np.random.Philox(key=[5152, 0]))
    pts = [random_patient(g, D, 70, "plain"), (np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32)),
           random_patient(g, D, 129, "missing")]
    th = np.stack([synth.theta(5152, p, 7, Q, D, R) for p in range(3)])
    tp = [sample_points(g, D, np.arange(D), np.array([0.0, 200.0], np.float32), 40) for _ in range(3)]
    ctx = make_ctx(7, Q, D, R, pts)
    out, st = ctx.posterior([0, 1, 2], th, [x[0] for x in tp], [x[1] for x in tp])
    ctx.close()
    assert st[1] == -1 and st[0] == 0 and st[2] == 0, st
    assert all(np.all(np.isnan(a)) for a in out[1])
    for p in (0, 2):
        ref = restate(7, Q, D, R, *pts[p], th[p], *tp[p])
        check_posterior(7, D, th[p], tp[p][0], ref, *out[p])


# ---------------------------------------------------------------------------------------------------------------------------
# jitter retries: the first k factorisation attempts of every entry count as failed (test hook); the outputs are those of the
# factor of K + k diag(sigma^2), var adds the test point's noise once; k = 11 exhausts the reference's ten retries
# ---------------------------------------------------------------------------------------------------------------------------
def _scaled_noise(th, D, k):
    th2 = th.copy()
    th2[:D] += 0.5 * np.log1p(k)
    return th2


@pytest.mark.parametrize("multi_cu", ["-1", "1", None])
@pytest.mark.parametrize("fails", [1, 3, 11])
def test_jitter_retries_on_every_factor_output(fails, multi_cu, monkeypatch):
    monkeypatch.setenv("MEDGP_DEBUG_FAIL_ATTEMPTS", str(fails))
    if multi_cu is None:
        monkeypatch.delenv("MEDGP_MULTI_CU", raising=False)
    else:
        monkeypatch.setenv("MEDGP_MULTI_CU", multi_cu)
    D, Q, R = 3, 3, 2
    ns = (40, 300, 64, 150, 10, 200)     # size classes of 1, 3, 4 and 5 64-blocks, entries of n <= 64
    pts = [synth.patient(5153, p, D, n, interleave=(p == 3)) for p, n in enumerate(ns)]   # entry 3 in the caller's order
    th = np.stack([synth.theta(5153, p, 7, Q, D, R) for p in range(len(ns))])
    g = np.random.default_rng(fails)
    tp = [sample_points(g, D, pts[p][0], pts[p][1], k) for p, k in enumerate((30, 70, 1, 65, 12, 0))]
    ctx = make_ctx(7, Q, D, R, pts)
    slots = np.arange(len(ns))
    post, st_p = ctx.posterior(slots, th, [x[0] for x in tp], [x[1] for x in tp])
    nop, st_n = ctx.posterior(slots, th, [x[0] for x in tp], [x[1] for x in tp], parts=False)
    fpb_m2 = np.array([x[0][0] if len(x[0]) else 0 for x in tp], np.int32)
    fpb_t2 = np.array([x[1][0] if len(x[1]) else 50.0 for x in tp], np.float32)
    fb_mean, fb_var, st_fb = ctx.fit_predict_batch(slots, th, fpb_m2, fpb_t2)
    fac, st_f = ctx.factor_batch(slots, th, ns)
    nl, _, st_g = ctx.nlml_grad(slots, th, False, keep_factor=True)
    if fails > 10:
        for st in (st_p, st_n, st_fb, st_f, st_g):
            assert np.all(st == -1), st
        for p in range(len(ns)):
            assert all(np.all(np.isnan(a)) for a in post[p]) and all(np.all(np.isnan(a)) for a in nop[p][:2])
            with pytest.raises(medgp_amd.MedgpError):
                ctx.get_factor(p, ns[p])
        assert np.all(np.isnan(fb_mean)) and np.all(np.isnan(fb_var)) and np.all(np.isnan(nl))
        fm, fv, fs = ctx.fit_predict(1, th[1], tp[1][0], tp[1][1])
        assert fs == -1 and np.all(np.isnan(fm)) and np.all(np.isnan(fv))
        ctx.close()
        return
    for st in (st_p, st_n, st_fb, st_f, st_g):
        assert np.all(st == fails), st
    for p, (m, t, y) in enumerate(pts):
        ref = restate(7, Q, D, R, m, t, y, th[p], *tp[p], jitter_rounds=fails)
        check_posterior(7, D, th[p], tp[p][0], ref, *post[p])
        check_posterior(7, D, th[p], tp[p][0], ref, *nop[p])
        assert nop[p][2] is None
        rb = restate(7, Q, D, R, m, t, y, th[p], fpb_m2[p:p + 1], fpb_t2[p:p + 1], jitter_rounds=fails)
        check_posterior(7, D, th[p], fpb_m2[p:p + 1], rb, fb_mean[p:p + 1], fb_var[p:p + 1])
        # factor of K + (1 + k) diag(sigma^2) in the caller's order, and z = L^-1 y
        Lm, z = fac[p]
        Kj = O.gram(7, Q, D, R, m, t, _scaled_noise(th[p], D, fails))
        assert np.abs(Lm @ Lm.T - Kj).max() <= 1e-11 * np.abs(Kj).max(), p
        zr = np.linalg.solve(np.linalg.cholesky(Kj), y.astype(np.float64))
        assert np.abs(z - zr).max() <= 1e-9 * np.abs(zr).max(), p
        # nlml_grad(keep_factor) -> get_factor: alpha and L^-1 of the retried factor
        orc = O.nlml_grad(7, Q, D, R, m, t, y, _scaled_noise(th[p], D, fails), flag_grad=False, want_alpha=True, want_linv=True)
        assert abs(nl[p] - orc["nlml"]) <= 1e-10 * abs(orc["nlml"]), p
        alpha, linv, _ = ctx.get_factor(p, ns[p])
        assert_fp32_close(alpha, orc["alpha"], f"alpha {p}")
        assert_fp32_close(linv, orc["linv"], f"linv {p}")
    fm, fv, fs = ctx.fit_predict(1, th[1], tp[1][0], tp[1][1])
    assert fs == fails
    ref = restate(7, Q, D, R, *pts[1], th[1], *tp[1], jitter_rounds=fails)
    check_posterior(7, D, th[1], tp[1][0], ref, fm, fv)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------
# D > 32 and large n
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [32, 33, 64, 128])
def test_parity_wide_covariate_sets(D):
    Q, R = 3, 4
    g = np.random.Generator(np.random.Philox(key=[5154, D]))
    ns = (129, 300, 64, 2 * D + 1)
    pts = [random_patient(g, D, n, mode) for n, mode in zip(ns, ("plain", "missing", "shuffled", "plain"))]
    th = np.stack([synth.theta(5154, D + p, 7, Q, D, R) for p in range(len(ns))])
    tp = [sample_points(g, D, pts[p][0], pts[p][1], k) for p, k in enumerate((130, 65, 64, 100))]
    ctx = make_ctx(7, Q, D, R, pts)
    out, st = ctx.posterior(np.arange(len(ns)), th, [x[0] for x in tp], [x[1] for x in tp])
    ctx.close()
    assert np.all(st == 0)
    for p, (m, t, y) in enumerate(pts):
        ref = restate(7, Q, D, R, m, t, y, th[p], *tp[p])
        check_posterior(7, D, th[p], tp[p][0], ref, *out[p])
        absent = np.setdiff1d(np.arange(D), m)
        assert np.all(out[p][2][:, absent].view(np.uint32) == 0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_work_row_accumulators_are_budget_invariant(monkeypatch):
    """D = 64: the accumulators sit behind V in the work rows (stride ld*64 + D*64 per tile, ld per size class); one tile per
    launch chunk gives the same bits as one chunk per class"""
    D, Q, R = 64, 2, 2
    g = np.random.Generator(np.random.Philox(key=[5155, 0]))
    ns = (60, 200, 330, 129)
    pts = [random_patient(g, D, n, "plain") for n in ns]
    th = np.stack([synth.theta(5155, p, 7, Q, D, R) for p in range(len(ns))])
    tp = [sample_points(g, D, pts[p][0], pts[p][1], k) for p, k in enumerate((70, 129, 64, 65))]
    args = (np.arange(len(ns)), th, [x[0] for x in tp], [x[1] for x in tp])
    ctx = make_ctx(7, Q, D, R, pts)
    ref, st = ctx.posterior(*args)
    assert np.all(st == 0) and len(ctx.last_plan()) >= 3, ctx.last_plan()
    ctx.close()
    monkeypatch.setenv("MEDGP_POSTERIOR_BUDGET_GB", "1e-6")
    ctx = make_ctx(7, Q, D, R, pts)
    ch, st2 = ctx.posterior(*args)
    ctx.close()
    assert np.all(st2 == 0)
    for p in range(len(ns)):
        for k in range(3):
            assert np.array_equal(_bits(ch[p][k]), _bits(ref[p][k])), (p, k)
    p = 2
    check_posterior(7, D, th[p], tp[p][0], restate(7, Q, D, R, *pts[p], th[p], *tp[p]), *ref[p])


def test_priced_shape_look_ahead(monkeypatch):
    """the shape of the DESIGN pricing, D = 64, N = 4096 on the look-ahead route, points spread over every 64-row panel"""
    monkeypatch.setenv("MEDGP_MULTI_CU", "1")
    D, Q, R, N = 64, 3, 4, 4096
    m, t, y = synth.patient(5156, 0, D, N)
    th = synth.theta(5156, 0, 7, Q, D, R)
    g = np.random.default_rng(7)
    src = np.arange(0, N, 16) + g.integers(0, 16, size=N // 16)     # one training point in every 16 rows: all panels
    m2 = np.concatenate([m[src[::2]], g.integers(0, D, size=150)]).astype(np.int32)
    t2 = np.concatenate([t[src[::2]], g.uniform(-3.0, 203.0, size=150)]).astype(np.float32)
    ctx = make_ctx(7, Q, D, R, [(m, t, y)])
    out, st = ctx.posterior([0], th[None, :], [m2], [t2])
    assert {r for (_, _, r) in ctx.last_plan()} == {2}
    ctx.close()
    assert st[0] == 0
    check_posterior(7, D, th, m2, restate(7, Q, D, R, m, t, y, th, m2, t2), *out[0])


# ---------------------------------------------------------------------------------------------------------------------------
# interleaving with the other calls of a context
# ---------------------------------------------------------------------------------------------------------------------------
def test_posterior_interleaved_with_other_calls():
    D, Q, R = 4, 3, 2
    ns = (70, 200, 33, 140)
    pts = [synth.patient(5157, p, D, n) for p, n in enumerate(ns)]
    th = np.stack([synth.theta(5157, p, 7, Q, D, R) for p in range(len(ns))])
    g = np.random.default_rng(8)
    tp = [sample_points(g, D, pts[p][0], pts[p][1], k) for p, k in enumerate((65, 40, 1, 129))]
    args = (np.arange(len(ns)), th, [x[0] for x in tp], [x[1] for x in tp])
    ctx = make_ctx(7, Q, D, R, pts)
    ref, st = ctx.posterior(*args)
    assert np.all(st == 0)
    nl_ref, gr_ref, st_ref = ctx.nlml_grad([3, 1, 0], th[[3, 1, 0]], True)
    # while an asynchronous lane holds a gradient call
    H = th.shape[1]
    lane_th = ctx.pinned((3, H), np.float64); lane_th[:] = th[[3, 1, 0]]
    lane_nl = ctx.pinned((3,), np.float64)
    lane_gr = ctx.pinned((3, H), np.float64)
    lane_st = ctx.pinned((3,), np.int32)
    ctx.nlml_grad_async(0, np.array([3, 1, 0]), lane_th, True, lane_nl, lane_gr, lane_st)
    mid, st_mid = ctx.posterior(*args)
    ctx.wait(0)
    assert np.array_equal(st_mid, st) and np.array_equal(lane_st, st_ref)
    assert np.array_equal(lane_nl, nl_ref) and np.array_equal(lane_gr, gr_ref)
    # posterior -> nlml_grad(keep_factor) -> posterior: alpha / Linv are shared with the gradient path
    ctx.nlml_grad(np.arange(len(ns))[::-1], th[::-1], False, keep_factor=True)
    after, st_after = ctx.posterior(*args)
    assert np.array_equal(st_after, st)
    for p in range(len(ns)):
        for k in range(3):
            assert np.array_equal(_bits(mid[p][k]), _bits(ref[p][k])), (p, k)
            assert np.array_equal(_bits(after[p][k]), _bits(ref[p][k])), (p, k)
    ctx.close()
    for p in (0, 3):
        check_posterior(7, D, th[p], tp[p][0], restate(7, Q, D, R, *pts[p], th[p], *tp[p]), *ref[p])
