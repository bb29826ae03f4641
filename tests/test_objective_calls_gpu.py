"""The derivative calls (loo_grad, lgo_grad, forecast_grad, fisher_vec, hess_vec, posterior_jvp, posterior_vjp, the mean and basis
calls) and nlml_grad issue their launches through shared host helpers (medgp_capi.hip: launch_slabsum, launch_epilogue,
factor_run_templated, launch_kinv, launch_kdot, launch_tiles, ...).  Folding them there was to change nothing: every call of
tests/objective_calls_cases.py must return the BITS and make the launches, label by label, of the commit before the fold, recorded on
one MI355X in tests/golden/objective_calls_parent.npz by tests/golden/make_objective_calls_parent.py -- on the plans the cases claim
(family R: a ragged class of two entries, so the tile grids run with the odd entry stride and every tail with more than one entry).

The calls also share BUF_GVEC, the BUF_FI_* tables, lane 0's staging and the gradient buffer: made one after another on ONE
context they must give, call by call, the bits of a fresh context, and a second round on the warm context allocates nothing
(tests/test_inference_buffers_gpu.py holds the inference calls to the same).

test_cases_are_the_shapes_they_claim needs no GPU and carries no gpu mark."""
import os

import numpy as np
import pytest

from medgp_amd import synth
import objective_calls_cases as OC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "objective_calls_parent.npz")
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()     # NaNs compared as bytes


def _check_family(fam):
    g = golden()
    labels = [str(x) for x in g["labels"]]
    calls = OC.calls(fam)
    # 1. each call on a fresh context: the plan the case claims, the parent's bits, statuses and launch counts
    for cname, f in calls:
        ctx = OC.make_ctx(fam)
        arrs, counts, res, plan = OC.run_one(ctx, f)
        ctx.close()
        key = f"{fam}/{cname}/"
        assert plan == OC.PLAN[fam], (key, plan)
        want = [g[key + str(i)] for i in range(int(g[key + "n"]))]
        assert sorted(counts) == labels, key
        assert {k: counts[k] for k in labels} == dict(zip(labels, g[key + "counts"].tolist())), (key, counts)
        assert len(arrs) == len(want), key
        st = np.asarray(OC.statuses(cname, res))
        assert st.dtype == np.int32 and any(_bytes_equal(st, w) for w in want), (key, st)
        for i, (a, w) in enumerate(zip(arrs, want)):
            assert _bytes_equal(a, w), (key, i)
        assert any(np.isfinite(a).any() for a in arrs if a.dtype.kind == "f"), key
    # 2. the same calls one after another on one context: call by call the same bits; a second round allocates nothing
    ctx = OC.make_ctx(fam)
    for rnd in range(2):
        if rnd == 1:
            warm = ctx.alloc_stats()[1]
        for cname, f in calls:
            arrs = OC.run_one(ctx, f)[0]
            key = f"{fam}/{cname}/"
            for i, a in enumerate(arrs):
                assert _bytes_equal(a, g[key + str(i)]), (key, i, "round", rnd)
    assert ctx.alloc_stats()[1] == warm
    ctx.close()


def test_cases_are_the_shapes_they_claim():
    """no GPU work: the size classes of every family by the plan's rule (the GPU tests hold the library's own plan to the same list) --
    R has a class of two entries of different block counts; H = 270 > 256 in family B (two parts in the gradient epilogue), Q in
    9 .. 16 there; a permuted patient and a group of more than 64 in families A and R; the fixture holds every call of every family"""
    for fam, (_, ns) in OC.FAMILIES.items():
        assert OC.plan_of(ns) == OC.PLAN[fam], fam
    assert OC.PLAN["R"][0] == (2, 4) and sorted((n + 63) // 64 for n in OC.FAMILIES["R"][1]) == [1, 3, 4]   # ragged: 4 and 3 blocks
    assert all(c[0] == 1 for f in "AB" for c in OC.PLAN[f])
    assert synth.num_hyp(*OC.FAMILIES["B"][0]) == 270 and 9 <= OC.FAMILIES["B"][0][1] <= 16
    for fam, want in (("A", [40, 130, 70]), ("R", [40, 130, 200])):
        _, pts, th, Hs = OC.data(fam)
        assert [p[1].shape[0] for p in pts] == want and np.any(np.diff(pts[1][0]) < 0) and not np.any(np.diff(pts[0][0]) < 0)
        assert all(h.shape == (p[1].shape[0], OC.PB) for h, p in zip(Hs, pts))
    assert np.bincount(OC._groups([130])[0][3:]).max() > 64
    names = [c[0] for c in OC.calls("A")]
    assert len(names) == 23 and all([c[0] for c in OC.calls(f)] == names for f in OC.FAMILIES)
    g = golden()
    assert all(f"{f}/{n}/counts" in g and f"{f}/{n}/n" in g for f in OC.FAMILIES for n in names)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", sorted(OC.FAMILIES))
def test_bits_and_launches_of_the_parent(fam):
    _check_family(fam)
