"""k_wgrad leaves out the MFMA blocks of the chunks of U that are zero in all of a wave's rows (kernels_wgrad.h, wg_zero_chunks): the
products it no longer issues are exact zeros, so nlml, gradient and status must keep the BITS they had before -- on both one-workgroup
shapes and on the look-ahead route (both must leave exact zeros left of the diagonal of U's diagonal blocks), at both prefetch depths
(PF = 1: wg_phase1, PF = 2: the loop in k_wgrad's body), at the shapes of tests/wgrad_zero_work_cases.py.

The bits before: tests/golden/wgrad_zero_work_parent.npz, recorded on one MI355X from the commit before the skip by
tests/golden/make_wgrad_zero_work_parent.py (keys "<case>/<route>/nlml|grad|status"; the prefetch depth does not change the bits,
tests/test_nlml_budget_gpu.py::test_prefetch_depths_bit_identical).  The same results are held to the fp64 error budget of
tests/test_nlml_budget_gpu.py against the long-double truth, with that file's helpers and bound.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import test_nlml_budget_gpu as B
import wgrad_zero_work_cases as WC

CASES = WC.cases()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_zero_work_parent.npz")
ROUTES = ["wg44", "wg84", "la"]
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def run(case, route, deep, monkeypatch):
    B._env(monkeypatch, route, deep)
    out = B._run(case)
    plan, prof = out[5], out[6]
    assert prof["k_wgrad"][1] == len(plan) and prof["k_lauum"][1] == 0, (plan, prof)     # the tile kernel ran, not the generic pair kernels
    if route == "la":
        assert all(c[2] == 2 for c in plan if c[1] >= 2), plan
    else:
        assert all(c[2] == (0 if route == "wg44" else 1) for c in plan), plan
    return out


def test_cases_are_the_shapes_they_claim():
    """no GPU work: the case builder gives the sizes, output counts and the failing patient the tests below rely on"""
    by = {c["id"]: c for c in CASES}
    for Q in (5, 1):
        c = by[f"edges_Q{Q}"]
        assert [p[1].shape[0] for p in c["pts"]] == [64, 65, 130, 70] and c["Q"] == Q and c["fails"] == [3]
        assert np.bincount(c["pts"][2][0]).tolist() == [1, 64, 65]
    c = by["flush_D24"]
    assert c["pts"][0][1].shape[0] == 192 and np.bincount(c["pts"][0][0]).tolist() == [8] * 24
    c = by["pf2_D2"]
    assert len(c["pts"]) == 1 and c["pts"][0][1].shape[0] == 256 and np.bincount(c["pts"][0][0]).tolist() == [128, 128]


@pytest.mark.parametrize("deep", ["1", "2"], ids=lambda d: f"pf{d}")
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_bits_of_the_parent_and_budget(case, route, deep, monkeypatch):
    out = run(case, route, deep, monkeypatch)
    nlml, grad, st = out[:3]
    g = golden()
    key = f"{case['id']}/{route}/"
    assert np.array_equal(st, g[key + "status"]), (key, st, g[key + "status"])
    for p in case["fails"]:
        assert st[p] < 0, (key, p, st)
    ok = st >= 0
    assert ok.sum() == len(st) - len(case["fails"])
    # bitwise: compared as integers, so that -0.0 / +0.0 and NaN payloads count too
    assert np.array_equal(nlml[ok].view(np.int64), g[key + "nlml"][ok].view(np.int64)), (key, "nlml")
    assert np.array_equal(grad[ok].view(np.int64), g[key + "grad"][ok].view(np.int64)), (key, "grad")
    B._check(case, out)
