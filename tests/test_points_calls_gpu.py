"""The calls that take a CSR list of test points run their test-point side through shared helpers -- in medgp_capi.hip check_points,
upload_point_call, launch_pjvp_solve, for_solved_chunks, download_mean_var / download_mean_var64, launch_wgrad, in call_plan.h
scatter_entry_blocks, in capi.py _point_args, _per_point and _split.  Folding them there was to change nothing: every run of
tests/points_calls_cases.py must return the BITS (NaNs and statuses included), make the launches label by label and lay out the plan
of the commit before the fold, recorded on one MI355X with that commit's library AND capi.py in tests/golden/points_calls_parent.npz
by tests/golden/make_points_calls_parent.py.  The runs: three families (three size classes with a permuted patient; a ragged class of
two entries; SM with meta2 == NULL), 0 / 5 / 70 points per patient, a call without any point, each at the default
MEDGP_POSTERIOR_BUDGET_GB and under one that cuts the launch chunks (posterior_vjp and posterior_joint: between the two entries of a
class), one failed entry in the mean and basis objectives.

test_fixture_and_cases_are_what_they_claim needs no GPU and carries no gpu mark."""
import os

import numpy as np
import pytest

import objective_calls_cases as OC
import points_calls_cases as PC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "points_calls_parent.npz")
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()     # NaNs compared as bytes


def test_fixture_and_cases_are_what_they_claim():
    """no GPU work: the fixture holds every run the GPU test asks for, nothing else, and stays below 1 MiB; the cases have the plans,
    the point counts, the empty patient, the budgets and the failed entry they claim, and the recorded counts show the cuts"""
    g = golden()
    heads = {f"{f}/{b}/{n}/" for f, b, n in PC.RUNS}
    assert len(heads) == len(PC.RUNS) == 3 * (len(PC.CALL_NAMES) + 19) + len(PC.NONE_CALLS)
    want = {"labels"}
    for h in heads:
        want |= {h + "counts", h + "plan", h + "n"} | {h + str(i) for i in range(int(g[h + "n"]))}
    assert set(g) == want
    assert os.path.getsize(GOLDEN) < 1 << 20
    labels = [str(x) for x in g["labels"]]
    for fam in PC.FAMILIES:
        kf, pts, th, Hs = PC.data(fam)
        ns = [p[1].shape[0] for p in pts]
        assert tuple(ns) == PC.NS[fam] and max(ns) <= 200 and OC.plan_of(ns) == PC.PLAN[fam], fam
        assert [c[0] for c in PC.calls(fam)] == PC.CALL_NAMES
        x = PC.points(fam)
        assert sorted(t.shape[0] for t in x["t2"]) == [0, 5, 70] and tuple(t.shape[0] for t in x["t2"]) == PC.POINTS[fam]
        assert (x["m2"] is None) == (fam == "S") == (kf[0] != 7)
        assert any(np.any(np.diff(p) < 0) for p in x["prefix"] if p.size)        # the forecast call has to sort
        # the classes with points, by the plan's rule (largest first, the bucket of the 64-block count)
        blocks = sorted({next(j for j in range(32) if (1 << j) >= (n + 63) // 64) for n, m in zip(ns, PC.POINTS[fam]) if m})
        assert len(blocks) == PC.CLASSES_WITH_POINTS[fam], fam
        fm, (Hb, blam) = PC.failing(fam)
        assert np.array_equal(Hb[PC.FAILED][:, 2], Hb[PC.FAILED][:, 0]) and not blam[PC.FAILED, [0, 2]].any() and blam[1:].all(axis=0)[1:].all()
        assert (fm is None) == (fam == "S")
        if fm is not None:
            assert not fm[0][0].any() and fm[1][PC.FAILED, 1] == 0 and fm[1][1:].all()
    assert np.any(np.diff(PC.data("A")[1][1][0]) < 0) and PC.PLAN["R"][0] == (2, 4) and PC.PLAN["S"][0] == (2, 2)
    assert [c[0] for c in PC.calls("A", True)] == list(PC.NONE_CALLS) and all(t.size == 0 for t in PC.points("A", True)["t2"])
    # the two-entry classes of R and S hold the patients with 5 and 70 points: the entry budgets lie between the larger need and the sum
    for fam, ld in (("R", 256), ("S", 128)):
        joint = [nt * ld * 64 * 8 + (64 * nt) ** 2 * 8 + m * m * 4 for nt, m in ((2, 70), (1, 5))]
        vjp = [nt * 2 * ld * 64 * 8 for nt in (2, 1)]
        for call, need in (("posterior_joint", joint), ("posterior_vjp", vjp)):
            assert max(need) <= float(PC.ENTRY_BUDGET_GB[(fam, call)]) * 2 ** 30 < sum(need), (fam, call)
    assert float(PC.TILE_BUDGET_GB) * 2 ** 30 < 64 * 64 * 8
    # what the recorded launch counts say: the small budget cut chunks wherever a cut is possible, the statuses are the claimed ones
    for fam, budget, name in PC.RUNS:
        key = f"{fam}/{budget}/{name}/"
        assert g[key + "plan"].tolist() == [list(c) for c in PC.PLAN["A" if fam == "none" else fam]], key
        arrs = [g[key + str(i)] for i in range(int(g[key + "n"]))]
        st = np.zeros(3, np.int32)
        if name.split("/")[0] in ("mean_nlml_grad", "basis_nlml_grad") and not (fam == "S" and name.startswith("mean")):
            st[PC.FAILED] = -1
            assert any(a.dtype.kind == "f" and np.isnan(a).any() for a in arrs), key
        assert any(_bytes_equal(a, st) for a in arrs), key
        if budget == "small":
            lab = labels.index(PC.chunk_label(name))
            ns_, nd = int(g[key + "counts"][lab]), int(g[f"{fam}/default/{name}/counts"][lab])
            assert (ns_ > nd) == PC.cut_possible(fam, name), key
            if PC.chunk_label(name) != "k_pvjp_cot" and "joint" not in name:
                assert nd == PC.CLASSES_WITH_POINTS[fam], key
            if name.startswith("posterior_vjp") and PC.cut_possible(fam, name):
                assert ns_ == nd + (PC.NCOT if name.endswith("custom") else 1), key


@pytest.mark.gpu
@pytest.mark.parametrize("fam,budget", [(f, b) for f in PC.FAMILIES for b in PC.BUDGETS] + [("none", "default")])
def test_bits_launches_and_plans_of_the_parent(fam, budget):
    g = golden()
    labels = [str(x) for x in g["labels"]]
    for f, b, name in PC.RUNS:
        if (f, b) != (fam, budget):
            continue
        arrs, counts, plan, res = PC.run(fam, budget, name)
        key = f"{fam}/{budget}/{name}/"
        want = [g[key + str(i)] for i in range(int(g[key + "n"]))]
        assert plan == [tuple(c) for c in g[key + "plan"].tolist()], (key, plan)
        assert sorted(counts) == labels, key
        assert {k: counts[k] for k in labels} == dict(zip(labels, g[key + "counts"].tolist())), (key, counts)
        assert len(arrs) == len(want), key
        assert np.asarray(PC.statuses(name, res)).dtype == np.int32, key
        for i, (a, w) in enumerate(zip(arrs, want)):
            assert _bytes_equal(a, w), (key, i)
        assert fam == "none" or any(np.isfinite(a).any() for a in arrs if a.dtype.kind == "f"), key
