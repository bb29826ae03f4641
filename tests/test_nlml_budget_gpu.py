"""GPU sweeps that hold medgp_nlml_grad to an fp64 error budget against the long-double truth of tests/nlml_truth.py, on every
kernel variant the dispatcher can launch, over the hyper ranges a trained model reaches, with the time axis moved away from 0, and
at the sizes the benchmarks run at (N = 512 .. 4096: the "large" sweep at the end of the file).

Budget of a case (per patient) = M * max(E_a, E_b, E_c): the errors of three legitimate fp64 programs on the CPU (the oracle, the
float64 run of the truth code, the same with the device's cosine tables and blocked factorisation), M = nlml_truth.M_NLML /
M_GRAD from their observed spread.  Every gradient budget is below 2^-30, 64 times under one fp32 ulp: a
float temporary, an expf or a narrowed dt anywhere in the gradient kernels fails these tests (the 1e-6 bar of the parity tests
does not see them).  Status words must equal the oracle's.  The route of every call is asserted from last_plan / profile_read.

Measured on one MI355X (device error / budget, worst per sweep) -- see DESIGN.md section 3.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
import nlml_truth as T

VARIANT = T.variant_cases()
WIDE = T.wide_cases()
HYPER = T.hyper_cases()
TIME = T.time_cases()
LARGE = {c["id"]: c for c in T.large_cases()}

ROUTES = {      # name -> (MEDGP_MULTI_CU, MEDGP_CHOLINV_NW)
    "wg44": ("-1", "44"), "wg84": ("-1", "84"), "la": ("1", None), "auto": (None, None),
}


def _env(monkeypatch, route, deep=None, park=None):
    mc, nw = ROUTES[route]
    for k, v in (("MEDGP_MULTI_CU", mc), ("MEDGP_CHOLINV_NW", nw), ("MEDGP_WGRAD_DEEP", deep), ("MEDGP_LA_PARK", park)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))
    for k in ("MEDGP_V0", "MEDGP_NO_CLASSES", "MEDGP_DEBUG_FAIL_ATTEMPTS"):
        monkeypatch.delenv(k, raising=False)


def _blocks(n):
    return (max(n, 1) + 63) // 64


def _run(case, slots=None, profile=True):
    """one context, one call with gradient and one without.  Returns (nlml, grad, status, nlml-only, status, plan, profile)"""
    pts = case["pts"]
    kidx = case["kidx"]
    slots = np.arange(len(pts)) if slots is None else np.asarray(slots)
    th = np.stack([case["th"][s] for s in slots])
    ctx = medgp_amd.Context(kidx, case["Q"], case["D"], case["R"])
    try:
        ctx.reserve(len(pts), max(p[1].shape[0] for p in pts), len(slots))
        for s, (m, t, y) in enumerate(pts):
            ctx.set_patient(s, m if kidx == 7 else None, t, y)
        if profile:
            ctx.profile_enable(True)
            ctx.profile_reset()
        nlml, grad, st = ctx.nlml_grad(slots, th, True)
        plan = ctx.last_plan()
        prof = ctx.profile_read() if profile else None
        if profile:
            ctx.profile_enable(False)
        nlml0, _, st0 = ctx.nlml_grad(slots, th, False)
    finally:
        ctx.close()
    return nlml, grad, st, nlml0, st0, plan, prof


def _check(case, out, slots=None, budget_case=None):
    """device results of a call against the budget of budget_case (default: the case itself), patient by patient"""
    bc = budget_case or case
    slots = np.arange(len(case["pts"])) if slots is None else np.asarray(slots)
    _check_refs(case["id"], out, [(bc, int(s)) for s in slots])


def _check_refs(label, out, refs):
    """device results of a call, entry b against the budget of patient refs[b] = (case, patient)"""
    nlml, grad, st, nlml0, st0 = out[:5]
    assert len(refs) == len(nlml)
    for b, (bc, s) in enumerate(refs):
        rst, tn, tg, bn, bg = T.budget_of(bc, s)
        assert st[b] == rst and st0[b] == rst, (label, b, st[b], st0[b], rst)
        if rst < 0:
            continue
        en, eg = T.error_pair(nlml[b], grad[b], tn, tg)
        print(f"{label} entry {b} n={bc['pts'][s][1].shape[0]}: nlml {en:.2e} / {bn:.2e}, grad {eg:.2e} / {bg:.2e}")
        assert en <= bn, (label, b, "nlml", en, bn)
        assert eg <= bg, (label, b, "grad", eg, bg)
        assert nlml0[b] == nlml[b], (label, b, "the nlml-only path must return the same bits")


def _check_route(case, route, plan, prof, ns):
    """the path the call took: routes of the size classes (medgp_last_plan) and the kernels that ran (profile_read)"""
    v0 = case["Q"] > 16
    assert sum(c[0] for c in plan) == len(ns)
    multi = [c for c in plan if c[1] >= 2]
    if route == "wg44":
        assert all(c[2] == 0 for c in plan), plan
    elif route == "wg84":
        assert all(c[2] == 1 for c in plan), plan
    elif route == "la":
        assert multi and all(c[2] == 2 for c in multi), plan
    has_la = any(c[2] == 2 for c in plan)
    assert (prof["k_la_step"][1] > 0) == has_la, (plan, prof["k_la_step"])
    if has_la:      # one k_la_step launch per 64-wide step of every look-ahead class
        assert prof["k_la_step"][1] == sum(c[1] for c in plan if c[2] == 2), (plan, prof["k_la_step"])
    nclass = len(plan)
    if v0:          # Q > 16: the generic pair kernels, and only they
        assert prof["k_lauum"][1] == nclass and prof["k_gradbins"][1] == nclass and prof["k_wgrad"][1] == 0, prof
    else:
        assert prof["k_lauum"][1] == 0 and prof["k_gradbins"][1] == 0, prof
        assert prof["k_wgrad"][1] == nclass, (plan, prof["k_wgrad"])      # (one bracket per class; Q > 8 launches twice inside it)
        assert prof["k_assemble"][1] >= nclass, (plan, prof["k_assemble"])


@pytest.mark.parametrize("deep", ["1", "2"], ids=lambda d: f"pf{d}")
@pytest.mark.parametrize("route", ["wg44", "wg84", "la", "auto"])
@pytest.mark.parametrize("case", VARIANT, ids=lambda c: c["id"])
def test_variant_matrix_within_budget(case, route, deep, monkeypatch):
    """every Q instantiation x both prefetch depths x both one-workgroup shapes, the look-ahead route and default routing, with and
    without gradient, on ragged batches of one-, two- / three-, (four-) and five-block patients incl. n = 64, 65, 128, 129.
    The pf1 / pf2 legs force the prefetch depth with MEDGP_WGRAD_DEEP; which depth ran is not observable through the ABI (see
    test_prefetch_depths_bit_identical)."""
    ns = [p[1].shape[0] for p in case["pts"]]
    assert max(_blocks(n) for n in ns) == 5 and min(_blocks(n) for n in ns) == 1
    _env(monkeypatch, route, deep)
    out = _run(case)
    _check_route(case, route, out[5], out[6], ns)
    if 200 in ns and route != "auto":       # the three- and the four-block entry share a class: a ragged launch (odd entry stride)
        assert any(c[0] == 2 and c[1] == 4 for c in out[5]), out[5]
    _check(case, out)


@pytest.mark.parametrize("route", ["wg84", "la"])
@pytest.mark.parametrize("case", VARIANT, ids=lambda c: c["id"])
def test_prefetch_depths_bit_identical(case, route, monkeypatch):
    """README: MEDGP_WGRAD_DEEP=1 and =2 give the same bits, and the bits of the default -- on the same input.  Which k_wgrad
    instantiation a launch takes cannot be observed through the ABI (medgp_last_plan and medgp_profile_read do not tell
    k_wgrad<.., 1> from <.., 2>): that the switch selects it rests on run_pipeline_one (`pf = wgrad_deep >= 0 ? wgrad_deep : ...`,
    read at medgp_create).  A library whose PF = 2 variant alone is wrong fails this test and the pf2 legs of the variant matrix."""
    res = {}
    for name, deep in (("default", None), ("pf1", "1"), ("pf2", "2")):
        _env(monkeypatch, route, deep)
        res[name] = _run(case, profile=False)
    for name, r in res.items():
        assert np.array_equal(r[0], res["pf1"][0]) and np.array_equal(r[1], res["pf1"][1]) and np.array_equal(r[2], res["pf1"][2]), \
            (case["id"], route, name)


def test_la_park_switch_bit_identical_where_parking_engages(monkeypatch):
    """README: MEDGP_LA_PARK=0 gives the bits of the default.  The look-ahead schedule parks a sleeping workgroup only for a class
    of nbatch <= 8 equally large entries with 256 % nbatch == 0, on steps with more than 256 / nbatch tasks.  Eight entries of
    n = 768 (12 blocks): 32 < ntask = 1 + aux + 12 F row blocks + 11 look-ahead rows x 2 slices at steps k = 5..8, so the default
    run parks there and the MEDGP_LA_PARK=0 run does not.  (On the variant cases every look-ahead class has one entry or is ragged
    and nothing ever parks.)  That parking engaged cannot be observed through the ABI -- the launch gains one grid row, the launch
    count stays -- and rests on run_pipeline_one's rule as restated here.  No truth is needed: the two runs must agree bit for bit,
    and with the one-workgroup route to the parity bars."""
    from medgp_amd import synth
    D, Q, R, N, P = 3, 3, 2, 768, 8
    pts, th = synth.cohort(31, P, D, N, Q=Q, R=R)
    case = dict(id="park", kidx=7, Q=Q, D=D, R=R, pts=pts, th=list(th))
    res = {}
    for name, route, park in (("default", "la", None), ("nopark", "la", "0"), ("wg", "wg84", None)):
        _env(monkeypatch, route, None, park)
        res[name] = _run(case)
    plan, prof = res["default"][5], res["default"][6]
    assert plan == [(8, 12, 2)] and prof["k_la_step"][1] == 12, (plan, prof["k_la_step"])
    assert res["nopark"][5] == plan
    for i in range(3):
        assert np.array_equal(res["default"][i], res["nopark"][i]), i
    assert np.all(res["default"][2] == 0) and np.all(res["wg"][2] == 0)
    assert np.all(np.abs(res["default"][0] - res["wg"][0]) <= 1e-10 * np.abs(res["wg"][0]))
    g0, g1 = res["default"][1], res["wg"][1]
    assert np.all(np.abs(g0 - g1) <= 1e-6 * np.maximum(np.abs(g1), 1e-3 * np.abs(g1).max(axis=1, keepdims=True)))


def test_default_prefetch_depth_is_budgeted_too(monkeypatch):
    """default routing and default prefetch depth (what a caller gets) on three cases"""
    for case in (VARIANT[4], VARIANT[10], VARIANT[17]):
        _env(monkeypatch, "auto")
        out = _run(case)
        _check_route(case, "auto", out[5], out[6], [p[1].shape[0] for p in case["pts"]])
        _check(case, out)


@pytest.mark.parametrize("shape", ["split", "onepart"])
@pytest.mark.parametrize("route", ["wg44", "wg84", "la", "auto"])
@pytest.mark.parametrize("case", WIDE, ids=lambda c: c["id"])
def test_wide_hyper_vectors_both_epilogue_shapes(case, route, shape, monkeypatch):
    """H = 1114 and 2954: k_epilogue splits the hypers of an entry over workgroups when a size class has 2 * count < num_cu entries
    and takes one part per entry otherwise (the count is that of the CLASS, not of the call).  "split": the three patients once.
    "onepart": the three-block patient repeated num_cu / 2 times, so that its class alone reaches the threshold, plus the other two
    once (their classes stay split).  The shape is asserted from the class counts of medgp_last_plan."""
    import torch
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    ns = [p[1].shape[0] for p in case["pts"]]
    assert _blocks(ns[1]) == 3 and T.num_hyp(7, case["Q"], case["D"], case["R"]) > 256
    if shape == "split":
        slots = np.arange(len(ns))
    else:
        slots = np.array([0] + [1] * ((num_cu + 1) // 2) + [2])
    _env(monkeypatch, route)
    out = _run(case, slots)
    plan, prof = out[5], out[6]
    assert sum(c[0] for c in plan) == len(slots)
    if shape == "split":
        assert all(2 * c[0] < num_cu for c in plan), (plan, num_cu)
    else:       # the class of the repeated patient (three or four blocks) takes the one-part epilogue
        assert any(2 * c[0] >= num_cu and c[1] in (3, 4) for c in plan), (plan, num_cu)
    assert prof["k_epilogue"][1] == 2 * len(plan), (plan, prof["k_epilogue"])     # k_slabsum + k_epilogue per class
    if route == "la":
        assert all(c[2] == 2 for c in plan if c[1] >= 2), plan
    elif route != "auto":
        assert all(c[2] == (0 if route == "wg44" else 1) for c in plan), plan
    assert (prof["k_la_step"][1] > 0) == any(c[2] == 2 for c in plan)
    _check(case, out, slots)


@pytest.mark.parametrize("route", ["wg44", "la", "auto"])
@pytest.mark.parametrize("case", HYPER, ids=lambda c: c["id"])
def test_hyper_range_within_budget(case, route, monkeypatch):
    """corners of the hyper ranges x the patient modes same_time / burst / missing"""
    nbmax = max(_blocks(p[1].shape[0]) for p in case["pts"])
    assert nbmax >= 2       # every case has a patient of two or three blocks: forced, the look-ahead schedule takes it (no leg skips)
    _env(monkeypatch, route)
    out = _run(case)
    plan, prof = out[5], out[6]
    if route == "la":
        assert all(c[2] == 2 for c in plan if c[1] >= 2) and prof["k_la_step"][1] == sum(c[1] for c in plan if c[2] == 2), plan
    elif route == "wg44":
        assert all(c[2] == 0 for c in plan) and prof["k_la_step"][1] == 0, plan
    _check(case, out)


@pytest.mark.parametrize("off", T.TIME_OFFSETS, ids=lambda o: f"off{int(o)}")
@pytest.mark.parametrize("case", TIME, ids=lambda c: c["id"])
def test_time_axis_offset_within_unshifted_budget(case, off, monkeypatch):
    """times on a 2^-6 h grid moved by 0, 2^10, 2^14 h (exact in float32; 2^14 h is the documented limit of |t|): K depends on differences only, the truth is
    bit-identical, and the device must meet the budget of the UNSHIFTED case at every offset"""
    _env(monkeypatch, "auto")
    sh = T.shifted(case, off)
    out = _run(sh)
    _check(sh, out, budget_case=case)


# ---- the large sweep: N = 512 .. 4096 ---------------------------------------------------------------------------------------------------
# The truths of the patients of n > 1024 are committed (tests/golden/nlml_truth_large.npz, re-derived on the CPU by
# tests/test_nlml_truth.py); the others are computed on the host when first needed, about 100 s in all.

def test_large_headline_512_entries_default_routing(monkeypatch):
    """the benchmark's shape: 512 entries of n = 512, D = 24, Q = 5, R = 8 in one call on default routing.  More entries than CUs
    (asserted), so the dispatcher takes k_cholinv<4,4> (asserted from the plan: route 0), eight row blocks over its four block slots.
    That two such workgroups share a CU and that k_wgrad runs at its large-launch prefetch depth (PF = 1) cannot be observed through
    the ABI: both rest on run_pipeline_one's rules for a launch of more entries than CUs (see test_prefetch_depths_bit_identical).
    Eight distinct patients (plain, missing, shuffled) repeated 64 times: every entry within the budget of its patient, and the
    repeats of a patient bit-identical."""
    import torch
    assert torch.cuda.get_device_properties(0).multi_processor_count < 512
    case = LARGE["large_headline"]
    slots = np.tile(np.arange(8), 64)
    _env(monkeypatch, "auto")
    out = _run(case, slots)
    plan, prof = out[5], out[6]
    assert plan == [(512, 8, 0)], plan
    assert prof["k_la_step"][1] == 0 and prof["k_wgrad"][1] == 1 and prof["k_lauum"][1] == 0, prof
    _check(case, out, slots)
    for b in range(8, 512):
        assert out[0][b] == out[0][b % 8] and np.array_equal(out[1][b], out[1][b % 8]) and out[3][b] == out[3][b % 8], b


@pytest.mark.parametrize("route", ["wg44", "wg84", "la", "auto"])
def test_large_headline_batch_of_8(route, monkeypatch):
    """the same eight patients once: at most one patient per CU, on both one-workgroup shapes, the look-ahead route and default routing"""
    case = LARGE["large_headline"]
    _env(monkeypatch, route)
    out = _run(case)
    _check_route(case, route, out[5], out[6], [512] * 8)
    assert [c[:2] for c in out[5]] == [(8, 8)], out[5]
    _check(case, out)


SECOND_PASS = ["large_pass2", "large_q_Q8", "large_q_Q9", "large_q_Q16", "large_q_Q17", "large_sm_Q4", "large_se"]
ROUTE_DEPTH = [("wg44", None), ("wg84", "1"), ("wg84", "2"), ("la", "1"), ("la", "2"), ("auto", None)]


@pytest.mark.parametrize("route,deep", ROUTE_DEPTH, ids=lambda x: f"pf{x}" if x in ("1", "2") else (x or "pfauto"))
@pytest.mark.parametrize("cid", SECOND_PASS)
def test_large_second_pass_within_budget(cid, route, deep, monkeypatch):
    """more row blocks than k_cholinv<8,4> has slots: n = 513, 576 (nine blocks: the first block past the eight slots), 768 (a full
    second pass), 1024 (two full passes of <8,4>, four of <4,4>) in one ragged call; n = 640 (ten blocks) at Q = 8, 9, 16 (one and
    two launches of assembly and k_wgrad) and Q = 17 (generic pair kernels, no k_wgrad: _check_route); the single-output families SM
    (Q = 4) and SE at n = 1024.  Both prefetch depths on the wg84 and la legs."""
    case = LARGE[cid]
    ns = [p[1].shape[0] for p in case["pts"]]
    assert [_blocks(n) for n in ns] == {"large_pass2": [9, 9, 12, 16], "large_sm_Q4": [16], "large_se": [16]}.get(cid, [10])
    _env(monkeypatch, route, deep)
    out = _run(case)
    _check_route(case, route, out[5], out[6], ns)
    assert max(c[1] for c in out[5]) == max(_blocks(n) for n in ns), out[5]
    _check(case, out)


def test_large_parked_launch_within_budget(monkeypatch):
    """eight equal entries of n = 768 on the look-ahead route: the launch geometry with a parked workgroup (default) and without
    (MEDGP_LA_PARK=0), BOTH against the truth (test_la_park_switch_bit_identical_where_parking_engages knows only that they agree)"""
    big = LARGE["large_pass2"]
    assert big["pts"][2][1].shape[0] == 768
    case = dict(big, id="large_park", pts=[big["pts"][2]], th=[big["th"][2]])
    slots = np.zeros(8, np.int64)
    res = {}
    for name, park in (("default", None), ("nopark", "0")):
        _env(monkeypatch, "la", None, park)
        res[name] = out = _run(case, slots)
        assert out[5] == [(8, 12, 2)] and out[6]["k_la_step"][1] == 12, (name, out[5], out[6]["k_la_step"])
        _check_refs(f"large_park_{name}", out, [(big, 2)] * 8)
        for b in range(1, 8):
            assert out[0][b] == out[0][0] and np.array_equal(out[1][b], out[1][0]), (name, b)
    for i in range(3):
        assert np.array_equal(res["default"][i], res["nopark"][i]), i


LONG = [cid for cid in ("large_config3", "large_slices", "large_config5") if cid in LARGE]


@pytest.mark.parametrize("route", ["la", "wg84"])
@pytest.mark.parametrize("cid", LONG)
def test_large_long_chain_within_budget(cid, route, monkeypatch):
    """one patient of n = 2048 (32 look-ahead steps), n = 2880 (45: the steps k = 32 and k = 44, where la_slice_len changes, and
    la_fold off) and, where nlml_truth keeps it, n = 4096 at D = 64 (64), alone in its call: one k_la_step launch per 64-block on
    the look-ahead route, and the one-workgroup route <8,4> over the same matrix"""
    case = LARGE[cid]
    n = case["pts"][0][1].shape[0]
    nb = _blocks(n)
    assert len(case["pts"]) == 1 and nb == {"large_config3": 32, "large_slices": 45, "large_config5": 64}[cid]
    _env(monkeypatch, route)
    out = _run(case)
    plan, prof = out[5], out[6]
    assert plan == [(1, nb, 2 if route == "la" else 1)], plan
    assert prof["k_la_step"][1] == (nb if route == "la" else 0), prof["k_la_step"]
    _check_route(case, route, plan, prof, [n])
    _check(case, out)


@pytest.mark.parametrize("no_classes", [False, True], ids=["classes", "no_classes"])
def test_large_mixed_call_within_budget(no_classes, monkeypatch):
    """n = 2048 together with the eight n = 512 patients in one call on default routing: two size classes on forked streams, the
    large patient on the look-ahead route (asserted from the plan).  MEDGP_NO_CLASSES=1 (the documented switch back to one class
    per call, every entry at the leading dimension of the largest) is held to the same budgets."""
    small, big = LARGE["large_headline"], LARGE["large_config3"]
    assert (small["Q"], small["D"], small["R"]) == (big["Q"], big["D"], big["R"])
    case = dict(small, id="large_mixed", pts=small["pts"] + big["pts"], th=small["th"] + big["th"])
    refs = [(small, p) for p in range(8)] + [(big, 0)]
    _env(monkeypatch, "auto")
    if no_classes:
        monkeypatch.setenv("MEDGP_NO_CLASSES", "1")
    out = _run(case)
    plan, prof = out[5], out[6]
    assert sum(c[0] for c in plan) == 9, plan
    if no_classes:
        assert plan == [(9, 32, 2)], plan
    else:
        assert (1, 32, 2) in plan and sum(c[0] for c in plan if c[1] == 8) == 8, plan
    assert prof["k_la_step"][1] == sum(c[1] for c in plan if c[2] == 2), (plan, prof["k_la_step"])
    _check_refs(f"large_mixed_{'no_classes' if no_classes else 'classes'}", out, refs)
