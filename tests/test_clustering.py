"""Kernel clustering, CPU side: the C ABI's surface, the component features against the reference's
(tests/golden/clustering_ref.npz), the definition tests/gmm_ref.py against scikit-learn, the conditions under which the GPU test
(tests/test_clustering_gpu.py) may compare iteration counts and labels exactly, and the host logic of medgp_amd.clustering."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from medgp_amd import capi, clustering  # noqa: E402
import gmm_cases as GC  # noqa: E402
import gmm_ref as GR  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
ERR_ARG, ERR_NODEVICE = -1, -3


def test_abi_exports_gmm_fit(built_lib):
    lib = capi.load()
    assert lib.medgp_abi_version() >= 13
    assert hasattr(lib, "medgp_gmm_fit") and "medgp_gmm_fit" in capi.SYMBOLS


def _raw_fit(x, k, label0, max_iter=3, tol=0.0, reg=1e-6, n=None, d=None, nruns=None):
    lib = capi.load()
    x = np.ascontiguousarray(x, dtype=np.float64)
    k = np.ascontiguousarray(k, dtype=np.int32)
    label0 = np.ascontiguousarray(label0, dtype=np.int32)
    nr = k.shape[0] if nruns is None else nruns
    out_d = [np.zeros(max(nr, 1)) for _ in range(2)]
    out_i = [np.zeros(max(nr, 1), dtype=np.int32) for _ in range(2)]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    return lib.medgp_gmm_fit(0, x.shape[0] if n is None else n, x.shape[1] if d is None else d, x.ctypes.data_as(dp), nr,
                             k.ctypes.data_as(ip), label0.ctypes.data_as(ip), max_iter, tol, reg, out_d[0].ctypes.data_as(dp),
                             out_d[1].ctypes.data_as(dp), out_i[0].ctypes.data_as(ip), out_i[1].ctypes.data_as(ip), None, None, None, None, None)


def test_argument_errors(built_lib):
    lib = capi.load()
    x = np.random.default_rng(0).normal(size=(6, 2))
    l0 = np.array([[0, 1, 0, 1, 0, 1]])
    bad = [dict(n=1), dict(d=0), dict(d=GC.MAX_D + 1), dict(nruns=0), dict(max_iter=0), dict(tol=-1.0), dict(tol=float("nan")), dict(reg=-1e-6)]
    for kw in bad:
        assert _raw_fit(x, [2], l0, **kw) == ERR_ARG, kw
        assert b"medgp_gmm_fit" in lib.medgp_last_error(None)
    for k in (0, GC.MAX_K + 1, 7):                      # 7 > n = 6
        assert _raw_fit(x, [k], l0 * 0) == ERR_ARG, k
    assert _raw_fit(x, [2], l0 + 1) == ERR_ARG            # a label outside [0, K)
    assert _raw_fit(x, [2], -l0) == ERR_ARG
    assert lib.medgp_gmm_fit(0, 6, 2, None, 1, None, None, 3, 0.0, 0.0, None, None, None, None, None, None, None, None, None) == ERR_ARG
    if lib.medgp_device_count() <= 0:                     # a well-formed call: there is no CPU path to fall back to
        assert _raw_fit(x, [2], l0) == ERR_NODEVICE
        with pytest.raises(capi.MedgpError):
            capi.gmm_fit(x, [2], l0)
    with pytest.raises(ValueError):
        capi.gmm_fit(x, [2, 2], l0)                       # two runs, one row of labels


@pytest.mark.parametrize("fam", ["LMC-SM", "SM", "SE"])
def test_features_equal_the_references(fam):
    g = np.load(os.path.join(GOLD, "clustering_ref.npz"))
    key = fam.replace("-", "_")
    Q, D, R = (int(v) for v in g[key + "_QDR"])
    hyp = g[key + "_hyp"]
    pan, qidx, feat = clustering.extract_kernel_feature(fam, Q, D, R, np.arange(hyp.shape[0]), hyp)
    assert np.array_equal(pan, g[key + "_comp_pan"]) and np.array_equal(qidx, g[key + "_comp_qidx"])
    assert feat.shape == g[key + "_comp_feature"].shape
    assert feat.shape[0] == hyp.shape[0] * Q - 1          # the one switched-off component is dropped
    assert np.max(np.abs(feat - g[key + "_comp_feature"])) <= 1e-14
    with pytest.raises(NotImplementedError):
        clustering.extract_kernel_feature("Matern", Q, D, R, np.arange(hyp.shape[0]), hyp)


# ---- the definition against scikit-learn, and the conditions of the exact comparisons -----------------------------------------
@pytest.fixture(scope="module")
def spread():
    return {"vs_sklearn": dict.fromkeys(GR.KINDS, 0.0), "vs_permuted": dict.fromkeys(GR.KINDS, 0.0), "cases": 0, "sklearn_cases": 0}


_memo = {}


def definition(key, x, K, l0, max_iter, tol, reg):
    """(outputs, trace) of the definition for one run, computed once per module run and left unchanged"""
    if key not in _memo:
        trace = []
        _memo[key] = (GR.gmm_fit_one(x, K, l0, max_iter, tol, reg, trace=trace), trace)
    return _memo[key]


def _take(spread, which, got, ref):
    for kind in GR.KINDS:
        if kind in ref:
            spread[which][kind] = max(spread[which][kind], GR.rel_err(got[kind], ref[kind]))


def check_conditions(x, K, out, trace, tol):
    """What lets the GPU test compare n_iter, status and assign EXACTLY: no iteration decides within 1 % of tol, no point's two
    largest responsibilities are within 1e-6, every regularised covariance has cond <= 1e8."""
    assert out["status"] >= 0
    if tol > 0:
        assert all(abs(abs(ch) - tol) >= 0.01 * tol for ch, _ in trace), [ch for ch, _ in trace]
    if K > 1:
        r = np.sort(out["resp"], axis=1)
        assert np.min(r[:, -1] - r[:, -2]) > 1e-6
    assert max(c for _, c in trace) <= 1e8


@pytest.mark.parametrize("i", range(len(GC.CASES)), ids=[GC.case_id(c) for c in GC.CASES])
def test_definition_conditions_and_permutation_spread(i, spread):
    x, K, l0, max_iter, tol, reg = GC.case_data(i)
    out, trace = definition(("case", i), x, K, l0, max_iter, tol, reg)
    check_conditions(x, K, out, trace, tol)
    perm = np.random.default_rng([GC.SEED, i, 1]).permutation(x.shape[0])
    po = GR.gmm_fit_one(x[perm], K, l0[perm], max_iter, tol, reg)
    assert po["n_iter"] == out["n_iter"] and po["status"] == out["status"] and np.array_equal(po["assign"], out["assign"][perm])
    _take(spread, "vs_permuted", po, out)
    print(f"case {i}: n_iter {out['n_iter']} status {out['status']} cond {max(c for _, c in trace):.3g} permuted spread "
          + " ".join(f"{k} {GR.rel_err(po[k], out[k]):.3g}" for k in GR.KINDS))
    spread["cases"] += 1


def test_definition_against_stored_scikit_learn_results(spread):
    g = np.load(os.path.join(GOLD, "gmm_sklearn_cases.npz"))
    for i in g["cases"]:
        x, K, l0, max_iter, tol, reg = GC.case_data(int(i))
        assert np.array_equal(x, g[f"c{i}_x"]) and np.array_equal(l0, g[f"c{i}_label0"]), "the fixture was made from other cases"
        assert np.array_equal(g[f"c{i}_args"], [K, max_iter, tol, reg])
        out = definition(("case", int(i)), x, K, l0, max_iter, tol, reg)[0]
        assert out["n_iter"] == int(g[f"c{i}_n_iter"]) and out["status"] == int(g[f"c{i}_converged"])
        assert np.array_equal(out["assign"], g[f"c{i}_predict"])
        _take(spread, "vs_sklearn", out, {"lower_bound": g[f"c{i}_lower_bound"], "bic": g[f"c{i}_bic"], "weights": g[f"c{i}_weights"],
                                          "means": g[f"c{i}_means"]})
        spread["sklearn_cases"] += 1


def test_definition_against_scikit_learn_itself(spread):
    pytest.importorskip("sklearn")
    for i in range(len(GC.CASES)):
        x, K, l0, max_iter, tol, reg = GC.case_data(i)
        out = definition(("case", i), x, K, l0, max_iter, tol, reg)[0]
        sk = GR.sklearn_fit(x, K, l0, max_iter, tol, reg)
        assert out["n_iter"] == sk["n_iter"] and out["status"] == sk["status"] and np.array_equal(out["assign"], sk["assign"])
        _take(spread, "vs_sklearn", out, sk)
        print(f"case {i}: vs scikit-learn " + " ".join(f"{k} {GR.rel_err(out[k], sk[k]):.3g}" for k in GR.KINDS))
    for call in GC.CALLS:
        x, k, l0, max_iter, tol, reg = getattr(GC, call)()
        for r in range(len(k)):
            out = definition((call, r), x, int(k[r]), l0[r], max_iter, tol, reg)[0]
            if out["status"] < 0:
                continue
            sk = GR.sklearn_fit(x, int(k[r]), l0[r], max_iter, tol, reg)
            assert out["n_iter"] == sk["n_iter"] and out["status"] == sk["status"] and np.array_equal(out["assign"], sk["assign"])
            _take(spread, "vs_sklearn", out, sk)
            print(f"{call} run {r}: vs scikit-learn " + " ".join(f"{k_} {GR.rel_err(out[k_], sk[k_]):.3g}" for k_ in GR.KINDS))
    spread["sklearn_cases"] += len(GC.CASES)


# ---- host logic ----------------------------------------------------------------------------------------------------------------
def test_selection_rule_ties_and_failed_runs():
    k = [1, 1, 2, 2, 2, 3, 3]
    lb = np.array([-5.0, -5.0, -3.0, -2.0, np.nan, -1.0, -1.5])
    bic = np.array([100.0, 90.0, 80.0, 80.0, np.nan, 80.0, 10.0])
    st = np.array([1, 0, 1, 1, -1, 1, 1])
    best, per_k = clustering.select_model(k, lb, bic, st)
    # K = 1: a tie in the lower bound keeps the first run (bic 100); K = 2: run 3 (the failed run 4 is skipped); K = 3: run 5.
    # BIC 100 -> 80 -> 80: the strict < keeps K = 2
    assert per_k == [(1, 100.0), (2, 80.0), (3, 80.0)] and best == 3
    assert clustering.select_model([1, 2], [np.nan, np.nan], [np.nan, np.nan], [-1, -1]) == (None, [])
    best, per_k = clustering.select_model([2, 2], [np.nan, -7.0], [np.nan, 5.0], [-1, 1])
    assert best == 1 and per_k == [(2, 5.0)]


def test_run_clustering_top_passes_starts_in_a_fixed_order(capsys):
    feat = GC.blobs(np.random.default_rng(5), 40, 3, 2)
    seen = {}

    def fake_fit(x, k, label0, max_iter, tol, reg_covar, device, full):
        seen.update(x=x, k=k.copy(), label0=label0.copy(), max_iter=max_iter, tol=tol, reg=reg_covar, full=full)
        nr = k.shape[0]
        lb = -np.arange(nr, dtype=np.float64)              # the first restart of every K wins
        bic = np.where(k == 2, 1.0, 2.0).astype(np.float64)
        asg = np.tile(np.arange(x.shape[0]) % 2, (nr, 1)).astype(np.int32)
        asg[np.flatnonzero(k == 2)[0]] = 1 - asg[0]
        return lb, bic, np.ones(nr, np.int32), np.ones(nr, np.int32), None, None, None, asg, 0.0

    num, assign = clustering.run_clustering_top("gmm", feat, max_cluster_num=3, init_num=4, max_iter_num=77, seed=9, fit=fake_fit)
    assert np.array_equal(seen["k"], np.repeat([1, 2, 3], 4)) and seen["max_iter"] == 77 and seen["tol"] == 1e-3 and seen["reg"] == 1e-6
    rng = np.random.default_rng(9)
    want = np.stack([clustering.init_labels(feat, K, rng) for K in np.repeat([1, 2, 3], 4)])
    assert np.array_equal(seen["label0"], want) and seen["full"]
    assert num == 2 and np.array_equal(assign, 1 - np.arange(40) % 2)
    out = capsys.readouterr().out
    assert "BIC = 2.000000 for 1 clusters" in out and "BIC = 1.000000 for 2 clusters" in out and "BIC = 2.000000 for 3 clusters" in out


def test_init_labels_nearest_seed_first_on_ties():
    x = np.array([[0.0], [2.0], [1.0], [5.0]])

    class Fixed:
        def choice(self, n, size, replace):
            assert n == 4 and size == 2 and replace is False
            return np.array([1, 0])
    lab = clustering.init_labels(x, 2, Fixed())
    assert np.array_equal(lab, [1, 0, 0, 0])               # the point at 1.0 is as far from both seeds: the first seed (2.0) wins
    lab = clustering.init_labels(GC.blobs(np.random.default_rng(1), 30, 2, 3), 5, np.random.default_rng(2))
    assert lab.dtype == np.int32 and set(lab.tolist()) == set(range(5))      # every seed labels at least itself


def test_none_algorithm_and_one_dimensional_features():
    num, assign = clustering.run_clustering_top("None", np.zeros((7, 3)), max_cluster_num=3)
    assert num == 1 and np.array_equal(assign, np.zeros(7, dtype=int))
    with pytest.raises(NotImplementedError):
        clustering.run_clustering_top("kmeans", np.zeros((7, 3)), max_cluster_num=3)
    g = np.load(os.path.join(GOLD, "clustering_ref.npz"))
    feat = g["SE_comp_feature"]
    assert feat.ndim == 1
    num, assign = clustering.run_clustering_top("gmm", feat, max_cluster_num=2, init_num=3, fit=GR.gmm_fit)
    assert num in (1, 2) and assign.shape == feat.shape and set(assign.tolist()) <= set(range(num))
    again = clustering.run_clustering_top("gmm", feat, max_cluster_num=2, init_num=3, fit=GR.gmm_fit)
    assert again[0] == num and np.array_equal(again[1], assign)


def _selection_gaps(feature, max_k, init_num, seed):
    """the two best lower bounds of every K and the two best BICs of the selection, as relative gaps"""
    rng = np.random.default_rng(seed)
    ks = [K for K in range(1, max_k + 1) for _ in range(init_num)]
    l0 = np.stack([clustering.init_labels(feature, K, rng) for K in ks])
    lb, bic, _, st = GR.gmm_fit(feature, ks, l0, 2000, 1e-3, 1e-6)
    gaps, best_bic = [], []
    for K in range(1, max_k + 1):
        v = np.sort(lb[(np.asarray(ks) == K) & (st >= 0)])[::-1]
        # K = 1 has one start whatever the draw: its restarts are the same run
        if K > 1 and len(v) > 1:
            gaps.append((v[0] - v[1]) / max(1.0, abs(v[0])))
        best_bic.append(bic[np.flatnonzero(np.asarray(ks) == K)[np.argmax(lb[np.asarray(ks) == K])]])
    b = np.sort(best_bic)
    return gaps, (b[1] - b[0]) / max(1.0, abs(b[0]))


def test_planted_groups_are_recovered():
    rng = np.random.default_rng(11)
    truth = np.arange(300) % 3
    x = np.array([[0.0, 0.0], [9.0, 1.0], [-4.0, 8.0]])[truth] + rng.normal(size=(300, 2)) * 0.7
    num, assign = clustering.run_clustering_top("gmm", x, max_cluster_num=5, init_num=10, seed=0, fit=GR.gmm_fit)
    assert num == 3
    table = np.array([[np.sum((truth == a) & (assign == b)) for b in range(3)] for a in range(3)])
    assert np.all(np.sort(table, axis=1)[:, :2] == 0) and sorted(np.argmax(table, axis=1).tolist()) == [0, 1, 2]
    other = clustering.run_clustering_top("gmm", x, max_cluster_num=5, init_num=10, seed=1, fit=GR.gmm_fit)
    assert other[0] == 3                                    # another seed: other starts, the same partition up to relabelling
    assert len({(a, b) for a, b in zip(assign.tolist(), other[1].tolist())}) == 3


def test_end_to_end_experiment_meets_the_conditions(tmp_path):
    """The experiment tests/test_clustering_gpu.py runs end to end: every run of its one gmm_fit call meets the conditions, and
    neither a K's best lower bound nor the selection's best BIC is decided by less than 1e-9 relative."""
    cfg, pans, hyp = GC.make_clustering_experiment(tmp_path)
    kp, kh = clustering.read_train_kernel(np.array([f"S{k:03d}" for k in range(GC.E2E_SUBJECTS + 1)]), os.path.dirname(cfg).replace("cfg", "train"))
    assert np.array_equal(kp, pans) and np.array_equal(kh, hyp) and len(kp) == GC.E2E_SUBJECTS
    _, _, feat = clustering.extract_kernel_feature("LMC-SM", 3, 2, 2, kp, kh)
    rng = np.random.default_rng(0)
    for K in (1, 2, 3):
        for _ in range(10):
            l0 = clustering.init_labels(feat, K, rng)
            trace = []
            out = GR.gmm_fit_one(feat, K, l0, 2000, 1e-3, 1e-6, trace=trace)
            check_conditions(feat, K, out, trace, 1e-3)
    gaps, bic_gap = _selection_gaps(feat, 3, 10, 0)
    assert all(g > 1e-9 or g == 0.0 for g in gaps), gaps     # 0: two starts that led to the same labels, the same run twice
    assert bic_gap > 1e-9


@pytest.mark.parametrize("call", GC.CALLS)
def test_multi_run_calls_meet_the_conditions(call, spread):
    """The multi-run calls of the GPU test: every run that does not fail meets the conditions and enters the permutation spread;
    the two planted failures fail where they were planted (one at the start, one at a later iteration that is the same in every
    order of the points), and the shapes the calls were built for are there (a 2-iteration run beside runs that use all of
    max_iter, an empty class, runs stopping at different iterations on both sides of the default polling interval, more than 64
    runs)."""
    x, k, l0, max_iter, tol, reg = getattr(GC, call)()
    outs = []
    for r in range(len(k)):
        out, trace = definition((call, r), x, int(k[r]), l0[r], max_iter, tol, reg)
        outs.append(out)
        if out["status"] >= 0:
            check_conditions(x, int(k[r]), out, trace, tol)
            perm = np.random.default_rng([GC.SEED, r, 2]).permutation(x.shape[0])
            po = GR.gmm_fit_one(x[perm], int(k[r]), l0[r][perm], max_iter, tol, reg)
            assert po["n_iter"] == out["n_iter"] and po["status"] == out["status"] and np.array_equal(po["assign"], out["assign"][perm])
            _take(spread, "vs_permuted", po, out)
    spread["cases"] += 1
    nit, st = [o["n_iter"] for o in outs], [o["status"] for o in outs]
    if call == "mixed_call":
        assert (nit[1], st[1]) == (2, 1) and (nit[0], st[0]) == (max_iter, 0) and 1 not in l0[2] and k[2] == 3 and st[2] >= 0
    elif call == "failing_call":
        assert st == [0, -1, 0] and nit[1] == 0 and np.isnan(outs[1]["bic"])
    elif call == "bits_call":
        assert min(nit) == 2 and max(nit) > 8 and all(s == 1 for s in st)
    elif call == "many_runs_call":
        assert len(k) == 70 and all(s >= 0 for s in st) and set(k.tolist()) == {1, 2, 3, 4, 5}
        assert all((nit[r], st[r]) == (2, 1) for r in range(70) if k[r] == 1) and all(nit[r] == max_iter for r in range(70) if k[r] >= 3)
        assert (nit[69], st[69]) == (max_iter, 0) and (nit[65], st[65]) == (2, 1)      # the second workgroup of the per-run kernel holds both kinds
    elif call == "chunked_bits_call":
        assert x.shape[0] > 32 * 64 and all(s == 1 for s in st) and set(k.tolist()) == {1, 2, 3, 4}
        assert min(nit) == 2 and sum(v < 8 for v in nit) >= 2 and sum(v > 8 for v in nit) >= 2 and len(set(nit)) >= 4
    else:
        f = GC.LATE_FAILING_RUN
        assert reg == 0.0 and [s < 0 for s in st] == [r == f for r in range(len(k))] and 0 < f < len(k) - 1
        assert 1 <= nit[f] < max_iter and np.isnan(outs[f]["bic"])
        assert all(nit[r] == max_iter for r in range(len(k)) if r != f) and max(k[r] for r in range(len(k)) if r != f) >= 2
        for s in range(8):                                  # the failure does not depend on the order of the points
            perm = np.random.default_rng([GC.SEED, s, 3]).permutation(x.shape[0])
            po = GR.gmm_fit_one(x[perm], int(k[f]), l0[f][perm], max_iter, tol, reg)
            assert (po["status"], po["n_iter"]) == (-1, nit[f]), (s, po["status"], po["n_iter"])


def test_spread_is_recorded(spread):
    """The largest differences, relative to max(1, |ref|) per output kind, of the definition against scikit-learn and against
    itself on permuted points, over every input the GPU test compares with the definition (the cases and every run of the multi-run
    calls of tests/gmm_cases.py), are what the GPU test's bars are built from (gmm_ref.bound: 50 x the larger).
    tests/golden/gmm_spread.json holds the figures recorded with the cases' seed (MEDGP_RECORD_GOLDEN=1 rewrites it, and needs
    scikit-learn); any other run must see the same cases and stay inside the bars: two fp64 programs may differ between numpy
    builds by the summation-order factor the bars allow the device."""
    assert spread["cases"] == len(GC.CASES) + len(GC.CALLS) and spread["sklearn_cases"] > 0, "run the whole module: the spread is taken over every case"
    ids = [GC.case_id(c) for c in GC.CASES] + list(GC.CALLS)
    if os.environ.get("MEDGP_RECORD_GOLDEN") == "1":
        assert spread["sklearn_cases"] > len(GC.CASES), "recording needs scikit-learn itself"
        json.dump({"seed": GC.SEED, "cases": ids, "vs_sklearn": spread["vs_sklearn"], "vs_permuted": spread["vs_permuted"],
                   "what": "max |a - b| / max(1, |b|) per output kind over the cases and multi-run calls of tests/gmm_cases.py (fp64): gmm_ref against scikit-learn from "
                           "the same start, and gmm_ref on permuted points against itself"}, open(GR.GOLDEN, "w"), indent=1)
    rec = json.load(open(GR.GOLDEN))
    assert rec["seed"] == GC.SEED and rec["cases"] == ids
    for kind in GR.KINDS:
        big = max(rec["vs_sklearn"][kind], rec["vs_permuted"][kind])
        assert 0.0 < big < 1e-10, (kind, big)
        assert spread["vs_sklearn"][kind] <= GR.bound(kind) and spread["vs_permuted"][kind] <= GR.bound(kind), (kind, spread, rec)
