"""Child process of tests/test_clustering_gpu.py's bit-invariance test: runs gmm_cases.bits_call() as one call under the
environment it was started with and saves every output to the .npz named on the command line."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from medgp_amd import capi  # noqa: E402
import gmm_cases as GC  # noqa: E402

if __name__ == "__main__":
    x, k, l0, max_iter, tol, reg = GC.bits_call()
    out = capi.gmm_fit(x, k, l0, max_iter=max_iter, tol=tol, reg_covar=reg, full=True)
    np.savez(sys.argv[1], *out[:8])
