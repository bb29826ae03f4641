#!/usr/bin/env python3
"""Generates the committed fixtures of the kernel-clustering step (run where the reference tree and scikit-learn exist; the
tests need neither):

    python tests/golden/make_clustering_golden.py <root of the reference tree>

1. clustering_ref.npz    -- small trained-hyper arrays (LMC-SM Q=3 D=2 R=2 with one component switched off, SM Q=3 with one
   switched off, SE with one subject switched off) and what the REFERENCE's extract_kernel_feature returns for them
   (medgpc/clustering/feature_extraction.py:5-98 with medgpc/visualization/fastkernel.py): comp_qidx, the subject index of each
   component, comp_feature.  The two modules are loaded by path under stub parent packages, because the packages' __init__
   files pull in plotting and statistics libraries the step does not use, and with the two numpy aliases the reference's text
   still spells the old way (np.float_, np.infty).
2. gmm_sklearn_cases.npz -- for a handful of the fixed-start cases of tests/gmm_cases.py: the inputs and what scikit-learn's
   GaussianMixture.fit gives from that start (gmm_ref.sklearn_fit): lower_bound_, n_iter_, converged_, weights_, means_, bic,
   predict.  The GPU machine then has scikit-learn's numbers without scikit-learn.
Data only; this file is the only one that reads the reference.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gmm_cases as GC  # noqa: E402
import gmm_ref as GR  # noqa: E402

SKLEARN_CASES = [7, 9, 11, 14, 15, 18, 23, 27]    # indices into gmm_cases.CASES


def load_reference(ref_root):
    if not hasattr(np, "float_"):
        np.float_ = np.float64
    if not hasattr(np, "infty"):
        np.infty = np.inf
    for name in ("medgpc", "medgpc.visualization", "medgpc.clustering"):
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules[name] = mod
    out = {}
    for name, rel in (("medgpc.visualization.fastkernel", "medgpc/visualization/fastkernel.py"),
                      ("medgpc.clustering.feature_extraction", "medgpc/clustering/feature_extraction.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref_root, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        out[name] = mod
    return out["medgpc.clustering.feature_extraction"]


def hypers(rng):
    P, Q, D, R = 40, 3, 2, 2
    lmc = GC.synthetic_hypers(rng, P, Q, D, R)
    # subject 5's component 1 switched off: A_1 = 0 and kappa_1 = exp(-40), so max |B_1| <= 1e-10
    lmc[5, D + 1 * D * R:D + 2 * D * R] = 0.0
    lmc[5, D + Q * (D * R + 2) + 1 * D:D + Q * (D * R + 2) + 2 * D] = -40.0
    sm = np.empty((P, 3 * Q + 1))
    sm[:, 0] = np.log(rng.uniform(0.15, 0.4, P))
    sm[:, 1:1 + Q] = np.log(rng.uniform(0.2, 1.5, (P, Q)))
    sm[:, 1 + Q:1 + 2 * Q] = np.log(1.0 / rng.uniform(12, 72, (P, Q)))
    sm[:, 1 + 2 * Q:] = np.log(1.0 / (2 * np.pi * rng.uniform(6, 72, (P, Q))))
    sm[7, 1 + 2] = -30.0          # weight exp(-30) <= 1e-10
    se = np.empty((P, 3))
    se[:, 0] = np.log(rng.uniform(0.15, 0.4, P))
    se[:, 1] = np.log(rng.uniform(6, 72, P))
    se[:, 2] = np.log(rng.uniform(0.5, 2.0, P))
    se[11, 2] = -20.0             # exp(2 * -20) <= 1e-10
    return {"LMC-SM": (lmc, Q, D, R), "SM": (sm, Q, 1, 1), "SE": (se, 1, 1, 1)}


def main(ref_root):
    fe = load_reference(ref_root)
    rng = np.random.default_rng(GC.SEED)
    out = {}
    for fam, (hyp, Q, D, R) in hypers(rng).items():
        pan = np.arange(hyp.shape[0])
        comp_pan, comp_qidx, comp_feature = fe.extract_kernel_feature(fam, Q, D, R, pan, hyp)
        key = fam.replace("-", "_")
        out[key + "_hyp"], out[key + "_QDR"] = hyp, np.array([Q, D, R])
        out[key + "_comp_pan"], out[key + "_comp_qidx"], out[key + "_comp_feature"] = comp_pan, comp_qidx, comp_feature
        print(fam, hyp.shape, "->", comp_feature.shape)
    np.savez_compressed(os.path.join(HERE, "clustering_ref.npz"), **out)
    import sklearn
    sk = {"sklearn_version": np.array(sklearn.__version__), "cases": np.array(SKLEARN_CASES)}
    for i in SKLEARN_CASES:
        x, K, l0, max_iter, tol, reg = GC.case_data(i)
        s = GR.sklearn_fit(x, K, l0, max_iter, tol, reg)
        sk[f"c{i}_x"], sk[f"c{i}_label0"], sk[f"c{i}_args"] = x, l0, np.array([K, max_iter, tol, reg], dtype=np.float64)
        sk[f"c{i}_lower_bound"], sk[f"c{i}_bic"] = np.array(s["lower_bound"]), np.array(s["bic"])
        sk[f"c{i}_n_iter"], sk[f"c{i}_converged"] = np.array(s["n_iter"]), np.array(s["status"])
        sk[f"c{i}_weights"], sk[f"c{i}_means"], sk[f"c{i}_predict"] = s["weights"], s["means"], s["assign"]
        print(GC.case_id(GC.CASES[i]), "n_iter", s["n_iter"], "converged", s["status"])
    np.savez_compressed(os.path.join(HERE, "gmm_sklearn_cases.npz"), **sk)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
