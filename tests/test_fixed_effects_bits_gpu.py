"""k_mean_small / k_basis_small and k_mean_post / k_basis_post run one body each (kernels_mean.h: fe_small_body, fe_post_body) behind a
column policy.  Sharing them was to change nothing: every call of tests/fixed_effects_cases.py must return the BITS, NaNs and statuses
included, of the commit before the bodies were shared, recorded on one MI355X in tests/golden/fixed_effects_parent.npz by
tests/golden/make_fixed_effects_parent.py.  The cases are those tests/test_objective_calls_gpu.py does not reach: 1, 17, 24, 33 and 64
columns, the posterior in FIXED mode, an improper entry, a failed pivot beside a legal zero column, an entry without test points.

test_fixture_and_cases_are_what_they_claim needs no GPU and carries no gpu mark."""
import os

import numpy as np
import pytest

import fixed_effects_cases as FC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fixed_effects_parent.npz")
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
    """no GPU work: the fixture holds every (case, call) the GPU test asks for, nothing else, and stays below 1 MiB; the cases have the
    column counts they claim (1, 24, 33, 64 for mean; 1, 17, 33, 64 and the 16 of the singular construction for basis), one entry
    without points, and the improper entry, the dependent flat pair and the zero column where the module says"""
    g = golden()
    keys = {f"{f}/{c}/{call}/n" for f, c in FC.CASES for call in FC.CALLS}
    assert keys <= set(g)
    assert set(g) == keys | {f"{k[:-1]}{i}" for k in keys for i in range(int(g[k]))}
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert sorted(FC.COLS["mean"].values()) == [1, 24, 33, 64] and sorted(FC.COLS["basis"].values()) == [1, 16, 17, 33, 64]
    for f, c in FC.CASES:
        s = FC.setup(f, c)
        nb = len(s["pts"])
        assert s["ncol"] == FC.COLS[f][c] and s["b0"].shape == s["lam"].shape == (nb, s["ncol"]), (f, c)
        assert [t.shape[0] for t in s["t2"]] == [0 if b == FC.EMPTY else 24 for b in range(nb)], (f, c)
        assert len({(p[1].shape[0] + 63) // 64 for p in s["pts"]}) > 1, (f, c)      # ragged
        if f == "basis":
            assert all(h.shape == (p[1].shape[0], s["ncol"]) for h, p in zip(s["H"], s["pts"]))
            assert all(h.shape == (t.shape[0], s["ncol"]) for h, t in zip(s["h2"], s["t2"]))
    s = FC.setup("mean", "lmc_D24")
    cnt = np.bincount(s["pts"][2][0], minlength=24)
    assert s["status"] == [0, 0, -1] and np.any((cnt == 0) & (s["lam"][2] == 0)) and not np.any((cnt == 0) & (s["lam"][0] == 0))
    s = FC.setup("basis", "singular")
    assert s["status"] == [0, 0, 0, -1, 0] and np.array_equal(s["H"][3][:, 15], s["H"][3][:, 0]) and not s["lam"][3, [0, 15]].any()
    assert not s["H"][4][:, 15].any() and s["lam"][4, 15] > 0
    # the statuses the parent returned: the failed entries under MARGINAL alone
    for f, c in (("mean", "lmc_D24"), ("basis", "singular")):
        want = np.array(FC.setup(f, c)["status"], np.int32)
        for call in FC.CALLS:
            arrs = [g[f"{f}/{c}/{call}/{i}"] for i in range(int(g[f"{f}/{c}/{call}/n"]))]
            assert any(_bytes_equal(a, want if "marginal" in call else np.zeros_like(want)) for a in arrs), (f, c, call)


@pytest.mark.gpu
@pytest.mark.parametrize("family,cid", FC.CASES, ids=[f"{f}-{c}" for f, c in FC.CASES])
def test_bits_of_the_parent(family, cid):
    g = golden()
    got = FC.run(family, cid)
    want_st = FC.setup(family, cid)["status"]
    for call in FC.CALLS:
        arrs, st = got[call]
        key = f"{family}/{cid}/{call}/"
        want = [g[key + str(i)] for i in range(int(g[key + "n"]))]
        assert len(arrs) == len(want), key
        assert st.dtype == np.int32 and list(st) == (want_st if "marginal" in call else [0] * len(want_st)), (key, st)
        for i, (a, w) in enumerate(zip(arrs, want)):
            assert _bytes_equal(a, w), (key, i)
        assert any(np.isfinite(a).any() for a in arrs if a.dtype.kind == "f"), key
