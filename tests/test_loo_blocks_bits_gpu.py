"""medgp_loo_batch and medgp_lgo_grad with groups of one, two and THREE 64-row blocks must return the BITS (NaNs and statuses included)
and make the launches, label by label, of the commit before their staged MFMA products and the block-column inverse were folded onto
panel_product / loo_block_column_inverse (kernels_posterior.h, kernels_loo.h): every accumulator kept its order of MFMAs.  The parent's
outputs were recorded on one MI355X in tests/golden/loo_blocks_parent.npz by tests/golden/make_loo_blocks_parent.py; the cases, and why
the N = 200 patient carries two group layouts, are in tests/loo_blocks_cases.py.  tests/test_objective_calls_gpu.py holds lgo_grad with
a group of 70 to the same; tests/test_loo_gpu.py and tests/test_lgo_grad_gpu.py hold the calls to their definitions.

test_cases_are_the_groups_they_claim needs no GPU and carries no gpu mark."""
import os

import numpy as np
import pytest

import loo_blocks_cases as LB
import objective_calls_cases as OC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loo_blocks_parent.npz")
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()     # NaNs compared as bytes


def test_cases_are_the_groups_they_claim():
    """no GPU work: family R, the group sizes of the N = 200 patient over the two layouts, the kept groups of the other two patients,
    members not contiguous, and a fixture that holds every call and stays small"""
    assert OC.FAMILIES[LB.FAM][1] == (40, 130, 200)
    sizes = {}
    for lay in LB.LAYOUTS:
        gs = LB.groups(lay)
        assert [g.shape[0] for g in gs] == [40, 130, 200] and all(g.dtype == np.int32 for g in gs)
        assert np.bincount(gs[1][gs[1] >= 0]).max() == 70 and (gs[1] == -1).sum() == 2
        g = gs[2]
        assert (g == -1).sum() == 1
        sizes[lay] = np.bincount(g[g >= 0]).tolist()
        big = np.flatnonzero(g == np.argmax(np.bincount(g[g >= 0])))
        assert np.any(np.diff(big) > 1)
    assert sizes["small"] == [1, 0, 2, 64, 65, 67] and sizes["large"] == [135, 64]
    names = [c[0] for c in LB.calls()]
    assert len(names) == 11 and len(set(names)) == 11
    g = golden()
    assert all(f"{n}/counts" in g and f"{n}/n" in g for n in names)
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "points_calls_parent.npz")) // 2


@pytest.mark.gpu
def test_bits_and_launches_of_the_parent():
    g = golden()
    labels = [str(x) for x in g["labels"]]
    for cname, f in LB.calls():
        ctx = OC.make_ctx(LB.FAM)
        arrs, counts, res, plan = OC.run_one(ctx, f)
        ctx.close()
        key = cname + "/"
        assert plan == OC.PLAN[LB.FAM], (key, plan)
        want = [g[key + str(i)] for i in range(int(g[key + "n"]))]
        assert sorted(counts) == labels, key
        assert {k: counts[k] for k in labels} == dict(zip(labels, g[key + "counts"].tolist())), (key, counts)
        assert len(arrs) == len(want), key
        st = np.asarray(LB.statuses(cname, res))
        assert st.dtype == np.int32 and any(_bytes_equal(st, w) for w in want), (key, st)
        for i, (a, w) in enumerate(zip(arrs, want)):
            assert _bytes_equal(a, w), (key, i)
        assert any(np.isfinite(a).any() for a in arrs if a.dtype.kind == "f"), key
