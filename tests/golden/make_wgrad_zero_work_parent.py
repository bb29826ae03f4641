#!/usr/bin/env python3
"""Writes wgrad_zero_work_parent.npz: nlml, gradient and status of the cases of tests/wgrad_zero_work_cases.py on the three
factorisation routes, as raw float64 / int32 arrays under the keys "<case>/<route>/nlml|grad|status".  Run by hand on an MI355X with
the library of the commit BEFORE k_wgrad skipped its zero chunks (a checkout of that commit, or MEDGP_LIB=<that build>):

    python tests/golden/make_wgrad_zero_work_parent.py [output.npz]

tests/test_wgrad_zero_work_gpu.py demands these bits of every later library.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import medgp_amd  # noqa: E402
import wgrad_zero_work_cases as WC  # noqa: E402

ROUTES = {"wg44": ("-1", "44"), "wg84": ("-1", "84"), "la": ("1", None)}     # as tests/test_nlml_budget_gpu.py


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "wgrad_zero_work_parent.npz")
    out = {}
    for k in ("MEDGP_WGRAD_DEEP", "MEDGP_LA_PARK", "MEDGP_V0", "MEDGP_NO_CLASSES", "MEDGP_DEBUG_FAIL_ATTEMPTS"):
        os.environ.pop(k, None)
    for case in WC.cases():
        for route, (mc, nw) in ROUTES.items():
            os.environ["MEDGP_MULTI_CU"] = mc
            os.environ.pop("MEDGP_CHOLINV_NW", None)
            if nw:
                os.environ["MEDGP_CHOLINV_NW"] = nw
            pts = case["pts"]
            ctx = medgp_amd.Context(case["kidx"], case["Q"], case["D"], case["R"])
            try:
                ctx.reserve(len(pts), max(p[1].shape[0] for p in pts), len(pts))
                for s, (m, t, y) in enumerate(pts):
                    ctx.set_patient(s, m, t, y)
                nlml, grad, st = ctx.nlml_grad(np.arange(len(pts)), np.stack(case["th"]), True)
            finally:
                ctx.close()
            key = f"{case['id']}/{route}/"
            out[key + "nlml"], out[key + "grad"], out[key + "status"] = np.asarray(nlml, np.float64), np.asarray(grad, np.float64), np.asarray(st, np.int32)
            print(key, "status", st.tolist(), "nlml", nlml.tolist(), flush=True)
    np.savez(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
