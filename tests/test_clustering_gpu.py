"""medgp_gmm_fit and medgp_amd.clustering on the GPU, through the C ABI.  The reference is the numpy definition tests/gmm_ref.py
(no scikit-learn here: its numbers come from tests/golden/gmm_sklearn_cases.npz).  Floating outputs are held to
B max(1, |ref|) per kind, B = gmm_ref.bound(kind) = 50 x the recorded fp64 spread (tests/golden/gmm_spread.json); n_iter, status
and assign are compared exactly -- tests/test_clustering.py asserts, on the CPU and for every input used here, the conditions
under which that is fair.  Each parity test prints its worst error beside B (pytest -s)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from medgp_amd import capi, clustering, cohort_mode  # noqa: E402
import gmm_cases as GC  # noqa: E402
import gmm_ref as GR  # noqa: E402

pytestmark = pytest.mark.gpu
OUT = ("lower_bound", "bic", "n_iter", "status", "weights", "means", "covs", "assign")
_ref_cache = {}


def reference(name, args):
    """the definition's outputs for a call, computed once and shared"""
    if name not in _ref_cache:
        x, k, l0, max_iter, tol, reg = args
        _ref_cache[name] = dict(zip(OUT, GR.gmm_fit(x, k, l0, max_iter, tol, reg, full=True)))
    return _ref_cache[name]


def device(args):
    x, k, l0, max_iter, tol, reg = args
    return dict(zip(OUT, capi.gmm_fit(x, k, l0, max_iter=max_iter, tol=tol, reg_covar=reg, full=True)))


def check_parity(tag, got, ref, kinds=GR.KINDS, runs=None):
    runs = np.arange(len(ref["status"])) if runs is None else np.asarray(runs)
    for key in ("n_iter", "status", "assign"):
        if key in ref:
            assert np.array_equal(got[key][runs], np.asarray(ref[key])[runs]), (tag, key, got[key][runs], np.asarray(ref[key])[runs])
    worst = {kind: GR.rel_err(got[kind][runs], np.asarray(ref[kind])[runs]) for kind in kinds}
    print(f"{tag}: " + "  ".join(f"{kind} {worst[kind]:.3g} (B {GR.bound(kind):.3g})" for kind in kinds))
    for kind in kinds:
        assert worst[kind] <= GR.bound(kind), (tag, kind, worst[kind], GR.bound(kind))


@pytest.mark.parametrize("i", range(len(GC.CASES)), ids=[GC.case_id(c) for c in GC.CASES])
def test_parity_with_the_definition(i, built_lib):
    x, K, l0, max_iter, tol, reg = GC.case_data(i)
    args = (x, np.array([K], dtype=np.int32), l0[None], max_iter, tol, reg)
    check_parity(GC.case_id(GC.CASES[i]), device(args), reference(("case", i), args))


def test_one_call_with_runs_of_mixed_k(built_lib):
    args = GC.mixed_call()
    got, ref = device(args), reference("mixed", args)
    assert (ref["n_iter"][1], ref["status"][1]) == (2, 1) and (ref["n_iter"][0], ref["status"][0]) == (args[3], 0)
    check_parity("mixed K", got, ref)
    kmax = int(args[1].max())
    for r, K in enumerate(args[1]):                         # entries beyond a run's K are zero
        assert np.all(got["weights"][r, K:] == 0) and np.all(got["means"][r, K:] == 0) and np.all(got["covs"][r, K:] == 0)
        assert got["weights"].shape[1] == kmax


def test_a_failed_run_does_not_touch_the_others(built_lib):
    args = GC.failing_call()
    got, ref = device(args), reference("failing", args)
    assert list(ref["status"]) == [0, -1, 0]
    assert got["status"][1] == -1 and np.isnan(got["lower_bound"][1]) and np.isnan(got["bic"][1]) and np.all(got["assign"][1] == -1)
    assert got["n_iter"][1] == ref["n_iter"][1] == 0
    check_parity("beside a failed run", got, ref, runs=[0, 2])
    x, k, l0, max_iter, tol, reg = args
    alone = device((x, k[[0, 2]], l0[[0, 2]], max_iter, tol, reg))      # ... to the bit: without the failing run, kmax 2
    for key in OUT:
        a, b = got[key][[0, 2]], alone[key]
        if key in ("weights", "means", "covs"):
            a = a[:, :2]
        assert a.tobytes() == b.tobytes(), key


def test_bits_do_not_depend_on_call_mates_order_or_polling(built_lib, tmp_path):
    assert "MEDGP_GMM_POLL" not in os.environ, "this test compares the default polling interval against 1"
    args = GC.bits_call()
    x, k, l0, max_iter, tol, reg = args
    got = device(args)
    check_parity("12 runs", got, reference("bits", args))
    assert got["n_iter"].max() > 8 and got["n_iter"].min() == 2          # runs freeze on both sides of the default interval
    rev = device((x, k[::-1], l0[::-1], max_iter, tol, reg))
    for key in OUT:
        assert rev[key][::-1].tobytes() == got[key].tobytes(), ("reversed", key)
    for r in (0, 3, 8):                                                   # alone: another kmax, so compare the run's own K entries
        one = device((x, k[r:r + 1], l0[r:r + 1], max_iter, tol, reg))
        K = int(k[r])
        for key in OUT:
            a, b = got[key][r], one[key][0]
            if key in ("weights", "means", "covs"):
                a = a[:K]
            assert np.ascontiguousarray(a).tobytes() == b.tobytes(), ("alone", r, key)
    # polling after every iteration, in a fresh process whose environment says so
    env = dict(os.environ, MEDGP_GMM_POLL="1")
    path = str(tmp_path / "poll1.npz")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gmm_bits_worker.py"), path], env=env, check=True, timeout=120)
    child = np.load(path)
    for j, key in enumerate(OUT):
        assert child[f"arr_{j}"].tobytes() == got[key].tobytes(), ("MEDGP_GMM_POLL=1", key)


def same_bits(tag, a, b, runs_a, runs_b, k):
    """runs runs_a of call a and runs runs_b of call b, the same runs in another company, agree to the bit; the calls may differ in
    kmax, so a run's own K entries of weights, means and covs are compared"""
    for ra, rb in zip(runs_a, runs_b):
        K = int(k[ra])
        for key in OUT:
            u, v = a[key][ra], b[key][rb]
            if key in ("weights", "means", "covs"):
                u, v = u[:K], v[:K]
            assert np.ascontiguousarray(u).tobytes() == np.ascontiguousarray(v).tobytes(), (tag, ra, key)


def test_more_runs_than_one_workgroup_of_the_tail(built_lib):
    """70 runs: the per-run kernel's second workgroup (runs 64 ... 69) and a grid of more than 64 in z"""
    args = GC.many_runs_call()
    x, k, l0, max_iter, tol, reg = args
    got = device(args)
    check_parity("70 runs", got, reference("many", args))
    assert got["n_iter"][65] == 2 and got["n_iter"][69] == max_iter
    same_bits("runs 64 ... 69 alone", got, device((x, k[64:], l0[64:], max_iter, tol, reg)), range(64, 70), range(6), k)
    same_bits("reversed", got, device((x, k[::-1], l0[::-1], max_iter, tol, reg)), range(70), range(69, -1, -1), k)


def test_bits_do_not_depend_on_call_mates_where_a_chunk_is_two_blocks(built_lib):
    args = GC.chunked_bits_call()
    x, k, l0, max_iter, tol, reg = args
    got = device(args)
    check_parity("6 runs on 2049 points", got, reference("chunked", args))
    assert got["n_iter"].max() > 8 and got["n_iter"].min() == 2          # runs freeze on both sides of the default polling interval
    same_bits("reversed", got, device((x, k[::-1], l0[::-1], max_iter, tol, reg)), range(6), range(5, -1, -1), k)
    for r in (0, 2):                                                      # one that stops before the first poll, one after the second
        same_bits("alone", got, device((x, k[r:r + 1], l0[r:r + 1], max_iter, tol, reg)), [r], [0], k)


def test_a_run_that_fails_after_the_start_freezes_alone(built_lib):
    args = GC.late_failing_call()
    x, k, l0, max_iter, tol, reg = args
    f = GC.LATE_FAILING_RUN
    got, ref = device(args), reference("late failing", args)
    mates = [r for r in range(len(k)) if r != f]
    assert [s < 0 for s in ref["status"]] == [r == f for r in range(len(k))] and 1 <= ref["n_iter"][f] < max_iter
    assert got["status"][f] == -1 and got["n_iter"][f] == ref["n_iter"][f]
    for key in ("lower_bound", "bic", "weights", "means", "covs"):
        assert np.all(np.isnan(got[key][f])), key
    assert np.all(got["assign"][f] == -1)
    check_parity("beside a run that fails at iteration %d" % ref["n_iter"][f], got, ref, runs=mates)
    same_bits("without the failing run", got, device((x, k[mates], l0[mates], max_iter, tol, reg)), mates, range(len(mates)), k)


def test_stored_scikit_learn_cases(built_lib):
    g = np.load(os.path.join(ROOT, "tests", "golden", "gmm_sklearn_cases.npz"))
    for i in (int(v) for v in g["cases"]):
        K, max_iter, tol, reg = g[f"c{i}_args"]
        args = (g[f"c{i}_x"], np.array([int(K)], dtype=np.int32), g[f"c{i}_label0"][None], int(max_iter), float(tol), float(reg))
        ref = {"lower_bound": g[f"c{i}_lower_bound"][None], "bic": g[f"c{i}_bic"][None], "n_iter": g[f"c{i}_n_iter"][None],
               "status": g[f"c{i}_converged"][None], "weights": g[f"c{i}_weights"][None], "means": g[f"c{i}_means"][None],
               "assign": g[f"c{i}_predict"][None]}
        check_parity(f"scikit-learn case {i}", device(args), ref, kinds=("lower_bound", "bic", "weights", "means"))


def test_capacity_is_a_host_check(built_lib, monkeypatch):
    x, K, l0, max_iter, tol, reg = GC.case_data(4)
    monkeypatch.setenv("MEDGP_GMM_BUDGET_GB", "1e-6")                    # one kilobyte
    with pytest.raises(capi.MedgpError) as e:
        capi.gmm_fit(x, [K], l0[None], max_iter=max_iter, tol=tol, reg_covar=reg)
    assert e.value.code == -4 and "MEDGP_GMM_BUDGET_GB" in str(e.value)
    monkeypatch.delenv("MEDGP_GMM_BUDGET_GB")
    assert capi.gmm_fit(x, [K], l0[None], max_iter=max_iter, tol=tol, reg_covar=reg)[3][0] >= 0


def test_end_to_end_mode_kernel_files(built_lib, tmp_path):
    """kernel_clustering_top on a small trained experiment writes the two files medgp_test reads, byte for byte what
    cohort_mode.output_mode_kernel writes when fed the assignment the numpy definition gives."""
    import json
    cfg, pans, hyp = GC.make_clustering_experiment(tmp_path / "exp")
    mode = clustering.kernel_clustering_top(cfg, fold=-1, algorithm="gmm", seed=0)
    exp = json.load(open(cfg))
    kdir = os.path.join(exp["exp_kernel_dir"], "all")
    got = {f: open(os.path.join(kdir, f), "rb").read() for f in ("gmm_mode_mixture_num.txt", "gmm_mode_param.bin")}
    cp, cq, feat = clustering.extract_kernel_feature("LMC-SM", exp["Q"], exp["D"], exp["R"], pans, hyp)
    num, assign = clustering.run_clustering_top("gmm", feat, max_cluster_num=exp["Q"], seed=0, fit=GR.gmm_fit)
    exp2 = dict(exp, exp_kernel_dir=str(tmp_path / "want"))
    want_mode = cohort_mode.output_mode_kernel(fold=-1, exp_param=exp2, pan_array=pans, hyp_array=hyp, mixture_pan=cp, mixture_index=cq,
                                               mixture_cluster_num=num, mixture_cluster_assign=assign, kernclust_alg="gmm")
    for f, b in got.items():
        assert b == open(os.path.join(str(tmp_path / "want"), "all", f), "rb").read(), f
    assert int(got["gmm_mode_mixture_num.txt"].split()[0]) == num and np.array_equal(mode, want_mode)
