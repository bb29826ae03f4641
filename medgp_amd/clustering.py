"""Kernel clustering, the step between training and the mode kernel: a response feature for every trained
spectral component, full-covariance Gaussian mixtures with K = 1 .. Q components chosen by BIC, and the hand-over of
(cluster_num, cluster_assign) to cohort_mode.output_mode_kernel.  ref: medgpc/clustering/kernclust.py:11-58,
feature_extraction.py:5-98, cluster.py:5-46, medgpc/util/binaryIO.py:20-35.  Function names and arguments are the reference's.

The EM runs of all K and all restarts are ONE medgp_gmm_fit call on the GPU (capi.gmm_fit; kernels_gmm.h).  What differs from the
reference: scikit-learn starts every restart from an unseeded k-means, so its selection is not reproducible; here every start is
init_labels (K distinct points drawn from a seeded generator, every point labelled with its nearest seed) and a call depends on
its arguments alone.  From a given start the EM is scikit-learn's (tests/gmm_ref.py is the definition, measured against it).

    python -m medgp_amd.clustering --cfg <exp_setup.json> --fold <k> --alg gmm [--seed 0] [--device 0]
"""
import argparse
import json
import os
from array import array

import numpy as np

from . import capi, cohort_mode

SCALE_THR = 1e-10      # components at or below this weight are not clustered (ref: feature_extraction.py:20, :40, :64)
FEATURE_LAGS = 72      # the response is sampled at lags 0 .. 71 hours (ref: feature_extraction.py:88)


def compute_sm_feature(mu, v):
    """ref: feature_extraction.py:87-98 with fastkernel.py:33-48.  The stationary response of a spectral-mixture component with
    frequency mu and spectral variance v at the lags tau = 0 .. 71, cos(2 pi tau mu) exp(-2 pi^2 v tau^2), followed by the
    periodic flag: 10 when mu > pi sqrt(v) (the oscillation outlives the envelope), else 0."""
    tau = np.arange(FEATURE_LAGS, dtype=np.float64)
    resp = np.exp(-2.0 * (np.pi ** 2) * (tau * tau * v)) * np.cos(2.0 * np.pi * (tau * mu))
    return np.hstack((resp, 10.0 if mu > np.pi * np.sqrt(v) else 0.0))


def _b_max(Q, D, R, hyp, q):
    """max |B_q|, B_q = A_q A_q^T + diag(kappa_q) (ref: medgpc/visualization/fastkernel.py:3-31; this reader takes A_q row by row,
    A_q[d, r] = hyp[D + q D R + d R + r])"""
    A = np.reshape(hyp[D + q * D * R:D + (q + 1) * D * R], (D, R))
    lam = np.exp(hyp[D + Q * (D * R + 2) + q * D:D + Q * (D * R + 2) + (q + 1) * D])
    return np.max(np.abs(A @ A.T + np.diag(lam)))


def extract_kernel_feature(kernel_type, Q, D, R, pan_array, hyp_array):
    """ref: feature_extraction.py:5-84.  Returns (comp_pan, comp_qidx, comp_feature): the subject, the component index and the
    feature of every component that is switched on.  'SE': one component per subject, the feature is the length scale (1-D);
    'SM' / 'LMC-SM': compute_sm_feature of (mu_q, v_q = exp(2 theta_v)), a component counting when its weight exp(theta_w)
    (SM) or max |B_q| (LMC-SM) exceeds 1e-10."""
    hyp_array = np.asarray(hyp_array, dtype=np.float64)
    comp_pan, comp_qidx, comp_feature = [], [], []
    if kernel_type == "SE":
        assert hyp_array.shape[1] == 3
        for pan, hyp in zip(pan_array, hyp_array):
            if abs(np.exp(2 * hyp[2])) > SCALE_THR:
                comp_pan.append(pan)
                comp_qidx.append(0)
                comp_feature.append(np.exp(hyp[1]))
    elif kernel_type == "SM":
        assert hyp_array.shape[1] == 3 * Q + 1
        for pan, hyp in zip(pan_array, hyp_array):
            for q in range(Q):
                if abs(np.exp(hyp[1 + q])) > SCALE_THR:
                    comp_pan.append(pan)
                    comp_qidx.append(q)
                    comp_feature.append(compute_sm_feature(np.exp(hyp[1 + Q + q]), np.exp(2 * hyp[1 + 2 * Q + q])))
    elif kernel_type == "LMC-SM":
        assert hyp_array.shape[1] == D + Q * (D * R + 2 + D)
        for pan, hyp in zip(pan_array, hyp_array):
            for q in range(Q):
                if _b_max(Q, D, R, hyp, q) > SCALE_THR:
                    comp_pan.append(pan)
                    comp_qidx.append(q)
                    comp_feature.append(compute_sm_feature(np.exp(hyp[D + Q * D * R + q]), np.exp(2 * hyp[D + Q * (D * R + 1) + q])))
    else:
        print("specified kernel type {} not supported".format(kernel_type))
        raise NotImplementedError
    return np.asarray(comp_pan), np.asarray(comp_qidx), np.asarray(comp_feature)


def init_labels(feature, K, rng):
    """The start of one EM run: K distinct points drawn with rng.choice are the seeds, every point gets the label of its nearest
    seed in squared distance (the first one on ties).  This stands where scikit-learn's unseeded k-means start stands in the
    reference (ref: cluster.py:34-37)."""
    feature = np.asarray(feature, dtype=np.float64)
    seeds = feature[rng.choice(feature.shape[0], size=K, replace=False)]
    d2 = ((feature[:, None, :] - seeds[None, :, :]) ** 2).sum(axis=2)
    return np.argmin(d2, axis=1).astype(np.int32)


def select_model(k, lower_bound, bic, status):
    """The reference's selection (ref: cluster.py:23-46 with scikit-learn's n_init): per K the run with the largest lower bound
    (the first on ties), then over K ascending the smallest BIC (strict <); failed runs (status < 0) are skipped.  Returns
    (index of the chosen run or None, [(K, bic of its best run)])."""
    k, best, lowest, per_k = np.asarray(k), None, np.inf, []
    for K in sorted(set(int(v) for v in k)):
        top = None
        for r in np.flatnonzero(k == K):
            if status[r] >= 0 and (top is None or lower_bound[r] > lower_bound[top]):
                top = int(r)
        if top is None:
            continue
        per_k.append((K, float(bic[top])))
        if bic[top] < lowest:
            lowest, best = bic[top], top
    return best, per_k


def run_clustering_top(algorithm, feature, max_cluster_num=None, init_num=10, max_iter_num=2000, seed=0, device=0, fit=None):
    """ref: cluster.py:5-46.  'None': one cluster.  'gmm': max_cluster_num x init_num starts drawn from
    np.random.default_rng(seed) in a fixed order (K ascending, restarts within K), ONE gmm_fit call for all of them, then
    select_model; the assignment is the chosen run's arg-max responsibility, like GaussianMixture.predict.  fit: a function with
    capi.gmm_fit's signature (the tests pass the numpy definition).  Returns (cluster_num, cluster_assign)."""
    if max_cluster_num is None:
        max_cluster_num = 5
        print("Warning: maximum number of clusters not set; use default value {}".format(max_cluster_num))
    algorithm = str(algorithm)
    feature = np.asarray(feature, dtype=np.float64)
    if algorithm == "None":
        print("Warning: clustering algorithm is not specified; skip clustering")
        return 1, np.zeros(feature.shape[0], dtype=np.int_)
    if algorithm != "gmm":
        print("Error: not supported algorithm {}".format(algorithm))
        raise NotImplementedError
    if feature.ndim == 1:          # SE: one number per subject
        feature = feature[:, None]
    rng = np.random.default_rng(seed)
    ks = [K for K in range(1, int(max_cluster_num) + 1) for _ in range(int(init_num))]
    label0 = np.stack([init_labels(feature, K, rng) for K in ks])
    fit = capi.gmm_fit if fit is None else fit
    lb, bic, _, st, _, _, _, assign, _ = fit(feature, np.asarray(ks, dtype=np.int32), label0, max_iter=max_iter_num, tol=1e-3,
                                             reg_covar=1e-6, device=device, full=True)
    best, per_k = select_model(ks, lb, bic, st)
    for K, b in per_k:
        print("BIC = {:.6f} for {} clusters".format(b, K))
    if best is None:
        raise RuntimeError("every mixture fit failed (singular covariance in all {} runs)".format(len(ks)))
    print("best cluster number using gmm clustering: {}".format(ks[best]))
    return ks[best], np.asarray(assign[best], dtype=np.int_)


def read_train_kernel(pan_array, kernel_dir):
    """ref: medgpc/util/binaryIO.py:20-35.  The subjects whose train_flag_<id>.txt is non-zero and their train_hyp_<id>.bin
    (native doubles); a subject with a missing or unreadable file is left out, as there."""
    valid_pan, valid_hyp = [], []
    for pan in pan_array:
        try:
            flag = np.atleast_1d(np.loadtxt(os.path.join(kernel_dir, "train_flag_{}.txt".format(pan)), dtype=int))[0]
            if flag:
                a = array("d")
                with open(os.path.join(kernel_dir, "train_hyp_{}.bin".format(pan)), "rb") as f:
                    a.frombytes(f.read())
                valid_pan.append(pan)
                valid_hyp.append(np.asarray(a))
        except Exception:
            continue
    return np.asarray(valid_pan), np.asarray(valid_hyp)


def kernel_clustering_top(exp_config, fold=-1, algorithm="gmm", seed=0, device=0, fit=None):
    """ref: kernclust.py:11-58, plotting off.  Reads the cohort and its trained kernels, extracts the component features, clusters
    them and writes the mode kernel through cohort_mode.output_mode_kernel (<alg>_mode_mixture_num.txt, <alg>_mode_param.bin).
    Like the reference, the chosen run's arg-max labels are passed on as they are: a selected model with a component that wins no
    point trips output_mode_*'s len(unique) == newQ assertion, here as there.  Returns the mode hypers."""
    exp_param = json.load(open(exp_config, "r"))
    cv_assign = np.atleast_1d(np.loadtxt(os.path.join(exp_param["cv_assign_file"]), dtype=int))
    valid_pan = np.atleast_1d(np.genfromtxt(os.path.join(exp_param["data_dir"], exp_param["cohort_id_list"]), dtype=str))
    if fold != -1:
        valid_pan = valid_pan[np.where(cv_assign != fold)]
    print("Info: # of ids available for this fold ({}): {}".format(fold, len(valid_pan)))
    kernel_pan, kernel_hyp = read_train_kernel(pan_array=valid_pan, kernel_dir=exp_param["exp_train_dir"])
    if len(kernel_pan) != len(valid_pan):
        print("Warning: # of valid trained subjects ({}) less than expected ({})".format(len(kernel_pan), len(valid_pan)))
    else:
        print("Info: successfully load all ids ({})".format(len(kernel_pan)))
    comp_pan, comp_qidx, comp_feature = extract_kernel_feature(kernel_type=exp_param["kernel"], Q=exp_param["Q"], D=exp_param["D"],
                                                               R=exp_param["R"], pan_array=kernel_pan, hyp_array=kernel_hyp)
    comp_cluster_num, comp_cluster_assign = run_clustering_top(algorithm=algorithm, feature=comp_feature,
                                                               max_cluster_num=exp_param["Q"], seed=seed, device=device, fit=fit)
    return cohort_mode.output_mode_kernel(fold=fold, exp_param=exp_param, pan_array=kernel_pan, hyp_array=kernel_hyp,
                                          mixture_pan=comp_pan, mixture_index=comp_qidx, mixture_cluster_num=comp_cluster_num,
                                          mixture_cluster_assign=comp_cluster_assign, kernclust_alg=algorithm, plotting_mode=0,
                                          device=device)


def main(argv=None):
    ap = argparse.ArgumentParser(description="kernel clustering and mode kernel of a trained cohort")
    ap.add_argument("--cfg", required=True)
    ap.add_argument("--fold", type=int, default=-1)
    ap.add_argument("--alg", default="gmm", choices=["gmm", "None"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    kernel_clustering_top(a.cfg, fold=a.fold, algorithm=a.alg, seed=a.seed, device=a.device)


if __name__ == "__main__":
    main()
