"""The fixed-start cases shared by tests/test_clustering.py (definition against scikit-learn; the conditions that keep exact
comparisons honest) and tests/test_clustering_gpu.py (device against the definition).  Data only: seeded numpy.

73-dimensional inputs are component features (medgp_amd.clustering.extract_kernel_feature on synthetic LMC-SM hypers, the
construction of tests/golden/clustering_ref.npz with more subjects); the others are Gaussian blobs.  Between them the cases use
every n of {2, 5, 63, 64, 65, 130, 300, 2049, 2112, 2113, 4100, 4161, 6200, 8257}, every d of {1, 2, 15, 16, 17, 33, 48, 49, 64, 73,
MAX_D}, every K of {1, 2, 3, 4, 5, MAX_K} and every stopping rule of {1, 3, 25 iterations, convergence at tol = 1e-3}.  The n above
2048 put more than one 64-point block into an M-step chunk (medgp_amd/csrc/gmm_tables.h: bpc = 2, 2, 2, 3, 3, 4, 5 in that
order, with last chunks of 1, 1, 2, 2, 3, 1, 5 blocks); d = 33 ... 64 are the padded widths 48 and 64."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from medgp_amd import clustering  # noqa: E402

SEED = 20261
MAX_D, MAX_K = 80, 16     # MEDGP_GMM_MAX_D, MEDGP_GMM_MAX_K (medgp_amd/csrc/gmm_tables.h)
CONV = (2000, 1e-3)       # the reference's max_iter with scikit-learn's default tol

# (n, d, K, max_iter, tol, reg_covar)
CASES = [
    (2, 1, 1, 3, 0.0, 1e-6), (2, 2, 2, 1, 0.0, 1e-6), (5, 1, 2, 3, 0.0, 1e-6), (5, 2, 1, 25, 0.0, 1e-6),
    (63, 15, 2, 3, 0.0, 1e-6), (64, 16, 2, 25, 0.0, 1e-6), (65, 17, 2, 1, 0.0, 1e-6), (65, 2, 5, *CONV, 1e-6),
    (130, 17, 5, 3, 0.0, 1e-6), (130, 73, 2, 25, 0.0, 1e-6), (130, 16, 1, 1, 0.0, 1e-6),
    (300, 73, 5, *CONV, 1e-6), (300, 73, 1, 3, 0.0, 1e-6), (300, MAX_D, 2, 3, 0.0, 1e-6), (300, MAX_D, 5, *CONV, 1e-3),
    (300, 2, MAX_K, 25, 0.0, 1e-6), (300, 15, MAX_K, 3, 0.0, 1e-3), (300, 1, 5, *CONV, 1e-6), (64, 2, MAX_K, *CONV, 1e-4),
    (63, 1, 1, *CONV, 1e-6),
    # cohort sizes: more than one 64-point block per M-step chunk (bpc = ceil(ceil(n / 64) / 32) > 1, short last chunks), and the
    # padded widths dp = 48 and 64
    (2049, 17, 2, 3, 0.0, 1e-6), (2113, 73, 2, *CONV, 1e-6), (2112, MAX_D, 2, 3, 0.0, 1e-6), (4161, 2, MAX_K, 25, 0.0, 1e-6),
    (8257, 33, 4, 3, 0.0, 1e-6), (300, 33, 2, 25, 0.0, 1e-6), (300, 48, 5, 3, 0.0, 1e-3), (130, 49, 2, 3, 0.0, 1e-6),
    (300, 64, 5, *CONV, 1e-6), (4100, 64, 2, 3, 0.0, 1e-6), (6200, 16, 3, 25, 0.0, 1e-6), (2113, 73, 4, *CONV, 1e-6),
]


def case_id(c):
    return "n{}_d{}_K{}_it{}_tol{:g}".format(*c[:5])


def synthetic_hypers(rng, P, Q=3, D=2, R=2):
    """Trained LMC-SM hypers of P subjects whose Q components fall into Q groups of period / length scale, so that the component
    features have structure for a mixture to find."""
    H = D + Q * (D * R + 2 + D)
    hyp = np.empty((P, H))
    hyp[:, :D] = np.log(rng.uniform(0.15, 0.4, (P, D)))
    hyp[:, D:D + Q * D * R] = rng.uniform(-1.5, 1.5, (P, Q * D * R)) * 0.9 / np.sqrt(Q * R)
    period = np.array([14.0, 30.0, 60.0, 22.0, 44.0])[:Q] * np.exp(rng.normal(size=(P, Q)) * 0.12)
    scale = np.array([60.0, 12.0, 30.0, 8.0, 45.0])[:Q] * np.exp(rng.normal(size=(P, Q)) * 0.12)
    hyp[:, D + Q * D * R:D + Q * D * R + Q] = np.log(1.0 / period)
    hyp[:, D + Q * D * R + Q:D + Q * D * R + 2 * Q] = np.log(1.0 / (2 * np.pi * scale))
    hyp[:, D + Q * (D * R + 2):] = np.log(rng.uniform(0.1, 0.5, (P, Q * D)) * 0.1 / Q)
    return hyp


def component_features(rng, n):
    """n component features [n, 73] of a synthetic LMC-SM cohort"""
    Q, D, R = 3, 2, 2
    P = (n + Q - 1) // Q
    hyp = synthetic_hypers(rng, P, Q, D, R)
    _, _, feat = clustering.extract_kernel_feature("LMC-SM", Q, D, R, np.arange(P), hyp)
    assert feat.shape == (P * Q, 73)
    return np.ascontiguousarray(feat[rng.permutation(P * Q)[:n]])


def blobs(rng, n, d, groups):
    centres = rng.normal(size=(groups, d)) * 5.0
    lab = np.arange(n) % groups
    return centres[lab] + rng.normal(size=(n, d)) * rng.uniform(0.6, 1.4, size=(1, d))


def case_data(i):
    """(x [n, d], K, label0 [n], max_iter, tol, reg_covar) of case i; the start is init_labels' (nearest of K drawn points)"""
    n, d, K, max_iter, tol, reg = CASES[i]
    rng = np.random.default_rng([SEED, i])
    x = component_features(rng, n) if d == 73 else blobs(rng, n, d, max(1, min(K, 4)))
    return x, K, clustering.init_labels(x, K, rng), max_iter, tol, reg


E2E_SEED, E2E_SUBJECTS = 3, 40
CALLS = ("mixed_call", "failing_call", "bits_call", "many_runs_call", "chunked_bits_call", "late_failing_call")   # the multi-run calls below


def make_clustering_experiment(root):
    """A small trained experiment on disk (40 subjects, LMC-SM Q = 3, D = 2, R = 2): synth_experiment.make_experiment plus what
    training leaves behind (train_hyp_<id>.bin, train_flag_<id>.txt; one subject failed) and the cohort files kernel_clustering_top
    reads.  Returns (path of exp_setup.json, ids of the trained subjects, their hypers)."""
    import json
    from medgp_amd import synth_experiment
    from medgp_amd.cohort_mode import write_double_to_bin
    rng = np.random.default_rng([SEED, E2E_SEED])
    pans = [f"S{k:03d}" for k in range(E2E_SUBJECTS + 1)]
    exp = synth_experiment.make_experiment(str(root), pans, D=2, Q=3, R=2, N=8)
    hyp = synthetic_hypers(rng, len(pans))
    for p, pan in enumerate(pans):
        flag = 0 if p == 4 else 1          # subject 4: training failed, no kernel
        np.savetxt(os.path.join(exp["dirs"]["train"], f"train_flag_{pan}.txt"), [flag], fmt="%d")
        if flag:
            write_double_to_bin(os.path.join(exp["dirs"]["train"], f"train_hyp_{pan}.bin"), hyp[p])
    cfg = json.load(open(exp["cfg"]))
    cfg["cohort_id_list"] = "cohort_ids.txt"
    cfg["cv_assign_file"] = os.path.join(exp["dirs"]["cfg"], "cv_assign.txt")
    np.savetxt(os.path.join(exp["dirs"]["data"], cfg["cohort_id_list"]), pans, fmt="%s")
    np.savetxt(cfg["cv_assign_file"], np.zeros(len(pans), dtype=int), fmt="%d")
    json.dump(cfg, open(exp["cfg"], "w"), indent=4)
    keep = np.array([p != 4 for p in range(len(pans))])
    return exp["cfg"], np.array(pans)[keep], hyp[keep]


def mixed_call():
    """One call with runs of mixed K on 130 blob points of dimension 2 (max_iter 6, tol 1e-3, reg 1e-6): a K = 1 run that
    converges in 2 iterations (its parameters never move) beside K = 5 runs that use all of max_iter, and a K = 3 start whose
    class 1 is empty.  Returns (x, k [nruns], label0 [nruns, n], max_iter, tol, reg_covar)."""
    rng = np.random.default_rng([SEED, 101])
    x = blobs(rng, 130, 2, 4) * np.array([[1.0, 0.4]])
    k = np.array([5, 1, 3, 2, 5, 3], dtype=np.int32)
    l0 = np.stack([rng.integers(0, K, 130).astype(np.int32) for K in k])
    l0[2] = np.where(l0[2] == 1, 2, l0[2])       # run 2: nobody starts in class 1
    l0[5] = clustering.init_labels(x, 3, rng)
    return x, k, l0, 6, 1e-3, 1e-6


def failing_call():
    """One call with reg_covar = 0 in which run 1 fails: its class 0 is two copies of the point at the origin, so the class mean
    is exactly 0, every difference is exactly 0 and the covariance's first pivot is exactly 0.  The other runs have well-conditioned
    classes and must be untouched.  Returns mixed_call()'s tuple."""
    rng = np.random.default_rng([SEED, 102])
    x = blobs(rng, 65, 2, 2)
    x[0] = x[1] = 0.0
    k = np.array([2, 3, 1], dtype=np.int32)
    l0 = np.stack([np.arange(65) % 2, np.r_[0, 0, 1 + np.arange(63) % 2], np.zeros(65)]).astype(np.int32)
    return x, k, l0, 5, 0.0, 0.0


def bits_call():
    """12 runs of mixed K on the 300 component features of the K = 5 convergence case, to convergence: they stop at different
    iterations, so freezing, polling and the other runs of the call all come into play."""
    i = [c[:3] for c in CASES].index((300, 73, 5))
    x = case_data(i)[0]
    rng = np.random.default_rng([SEED, 103])
    k = np.array([5, 1, 2, 3, 4, 5, 2, 3, 1, 4, 5, 2], dtype=np.int32)
    l0 = np.stack([clustering.init_labels(x, int(K), rng) for K in k])
    return x, k, l0, 2000, 1e-3, 1e-6


def many_runs_call():
    """70 runs in one call, K = 1 + r % 5, on mixed_call's kind of points with random starts (max_iter 6, tol 1e-3, reg 1e-6): more
    runs than one workgroup of the per-run kernel holds (64) and than any other call's grid has in z.  The K = 1 runs stop at
    iteration 2."""
    rng = np.random.default_rng([SEED, 104])
    x = blobs(rng, 130, 2, 4) * np.array([[1.0, 0.4]])
    k = (1 + np.arange(70) % 5).astype(np.int32)
    l0 = np.stack([rng.integers(0, K, 130).astype(np.int32) for K in k])
    return x, k, l0, 6, 1e-3, 1e-6


def chunked_bits_call():
    """6 runs of mixed K on the 2049 points of the first case with two blocks per M-step chunk, to convergence: bits_call's
    shape (runs stopping at different iterations, on both sides of the default polling interval) where a chunk is more than one
    block.  The first two draws of the K = 3 start decide within 1.2 % of tol; the third is used."""
    i = [c[:3] for c in CASES].index((2049, 17, 2))
    x = case_data(i)[0]
    rng = np.random.default_rng([SEED, 105])
    k = np.array([2, 1, 4, 3, 2, 4], dtype=np.int32)
    l0 = np.stack([clustering.init_labels(x, int(K), rng) for K in k])
    for _ in range(2):
        l0[3] = clustering.init_labels(x, 3, rng)
    return x, k, l0, 2000, 1e-3, 1e-6


LATE_FAILING_RUN = 2


def late_failing_call():
    """One call with reg_covar = 0 in which run LATE_FAILING_RUN fails AFTER the start: 130 standard-normal points in 2 dimensions
    of which the first two are copies of (50, 50), K = 2, and a start with points 0 ... 4 in class 0.  The covariance of class 0
    is regular at the start; EM then gives the far pair a class of its own, whose covariance is exactly 0.  Its mates, before
    and after it, go on to max_iter = 5: K = 1, and K = 2 from starts that halve the bulk (by parity of the index, by the sign
    of the first coordinate), which keep the pair inside a large class for those 5 iterations (they would isolate it later)."""
    rng = np.random.default_rng([SEED, 106])
    x = rng.normal(size=(130, 2))
    x[0] = x[1] = 50.0
    k = np.array([1, 2, 2, 2, 1], dtype=np.int32)
    l0 = np.stack([np.zeros(130), np.arange(130) % 2, np.r_[np.zeros(5), np.ones(125)], x[:, 0] > np.median(x[:, 0]), np.zeros(130)]).astype(np.int32)
    return x, k, l0, 5, 0.0, 0.0
