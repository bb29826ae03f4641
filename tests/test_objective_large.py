"""The large sweep of the four gradient objectives (objective_large.py) on the CPU: the committed fixture holds exactly the entries
the case list demands, every entry is bound to inputs rebuilt from seeds, the budget conditions (caps, cond(K)) hold on the stored
errors of the CPU programs, the cheap entries reproduce their stored bits, and the float64 run of the truth code stays within the
budget it helps to set.  No device output is read anywhere."""
import os

import numpy as np
import pytest

import forecast_grad_truth as FG
import nlml_truth as T
import objective_large as OL

X = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ids(es):
    return [OL.key_of(e) for e in es]


def test_case_list_and_fixture_keys():
    """every required leg is there with its sizes; what may be left out is a condition; the fixture holds exactly these keys"""
    E = OL.entries()
    assert len(set(_ids(E))) == len(E)
    assert len(OL.DROPPED) <= 2 and not any(cid == "large_pass2" for cid, _, _ in OL.DROPPED)
    assert OL.LONG_ABSENT <= set(OL.LONG_OPTIONAL)
    assert set(OL.all_entries()) - set(E) == {e for e in OL.all_entries() if e[1:4] in OL.DROPPED or e[1:] in OL.LONG_ABSENT}
    for (cid, p, obj), k in OL.DRAWS.items():
        assert obj in OL.OBJECTIVES and 0 <= k < 8 and k != T._draw(cid, p) and 0 <= p < len(OL.base_case(cid)["pts"])
    ns = {cid: [OL.n_of(cid, p) for p in range(len(OL.base_case(cid)["pts"]))] for cid in OL.CASE_ORDER}
    assert ns == {"large_pass2": [513, 576, 768, 1024], "large_q_Q8": [640], "large_q_Q9": [640], "large_q_Q16": [640],
                  OL.WIDE_ID: [200], "large_sm_Q4": [1024], "large_se": [1024], "large_config3": [2048]}
    assert [OL.fam(OL.base_case(c)) for c in OL.CASE_ORDER] == [(7, 3, 3, 2), (7, 8, 3, 2), (7, 9, 3, 2), (7, 16, 3, 2), (7, 2, 64, 2),
                                                                (8, 4, 1, 0), (0, 1, 1, 0), (7, 5, 24, 8)]
    m = OL.base_case(OL.WIDE_ID)["pts"][0][0]
    assert len(np.unique(m)) < 64 and m.max() > 32                       # mode "missing": covariates without observations
    per = {}
    for leg, cid, p, obj, tab in E:
        per.setdefault((leg, obj), []).append((cid, p, tab))
    want4 = [("large_pass2", p) for p in range(4)]
    for obj, tabs in (("loo", ["-"]), ("fisher", ["v2"]), ("fc", ["h0", "h6", "h48"]), ("lgo", ["cov", "win"])):
        assert {(c, p, t) for c, p, t in per[("pass2", obj)]} >= {(c, p, t) for c, p in want4 for t in tabs}
        for leg, cids in (("qsplit", ["large_q_Q8", "large_q_Q9", "large_q_Q16"]), ("wideD", [OL.WIDE_ID]), ("single", ["large_sm_Q4", "large_se"])):
            if leg == "single" and obj == "lgo":
                continue
            got = {(c, p, t) for c, p, t in per[(leg, obj)]}
            assert got >= {(c, 0, t) for c in cids if (c, 0, obj) not in OL.DROPPED for t in tabs}, (leg, obj)
    assert {("large_pass2", 1, "one"), ("large_pass2", 3, "max"), ("large_pass2", 3, "cap960")} <= set(per[("pass2", "lgo")])
    assert ("large_q_Q9", 0, "two320") in per[("qsplit", "lgo")]
    assert per[("long", "loo")] == [("large_config3", 0, "-")] and per[("long", "fisher")] == [("large_config3", 0, "v1")]
    z = OL.fixture()
    assert {str(k) for k in z["keys"]} == set(_ids(E))
    assert all(z[f"grad_hi_{i}"].size <= 2 * 1114 for i in range(len(z["keys"])))
    assert os.path.getsize(OL.FIXTURE) < 1 << 20


def test_tables_are_what_the_legs_are_about():
    """the 48 h bands reach over four 64-blocks at n = 1024; the large-group tables have the sizes they are named for; the group
    limit mirrors inference_tables.h"""
    pf = OL.table_of(("pass2", "large_pass2", 3, "fc", "h48"))
    band = np.arange(1024) - pf
    assert np.all(pf >= 0) and band.max() >= 256 and np.median(band) >= 128
    assert (np.arange(1024) - OL.table_of(("pass2", "large_pass2", 3, "fc", "h6"))).max() >= 32
    t = OL.case("large_pass2", "fc")["pts"][3][1]
    m = OL.case("large_pass2", "fc")["pts"][3][0]
    assert np.all(np.diff(t) >= 0) and np.any(np.diff(m) < 0)            # time order, covariates interleaved
    g, ng = OL.group_table("large_q_Q9", 0, "two320")
    assert ng == 2 and list(np.bincount(g)) == [320, 320] and np.any(np.diff(np.flatnonzero(g == 0)) > 1)
    g, ng = OL.group_table("large_pass2", 1, "one")
    assert ng == 1 and g.shape == (576,) and not g.any()
    with open(os.path.join(ROOT, "medgp_amd", "csrc", "inference_tables.h")) as f:
        src = f.read()
    assert "return 2 * mpad * mpad + 2 * mpad;" in src and "if (need > budget)" in src      # what loo_block_bytes / group_limit restate
    # the default budget of 2 GiB admits a group of 11584 rows: at n = 1024 the largest single group is the whole patient and there
    # is no row to add.  Under 15 MiB the limit is 960 rows: 960 in one group, 64 singletons, and one row more is refused.
    assert OL.group_limit(OL.DEFAULT_POSTERIOR_BUDGET) == 11584 and OL.loo_block_bytes(11585) > OL.DEFAULT_POSTERIOR_BUDGET
    g, ng = OL.group_table("large_pass2", 3, "max")
    assert ng == 1 and g.shape == (1024,) and OL.one_past("large_pass2", 3, "max") is None
    cap = int(OL.CAP_BUDGET_GB * 1073741824.0)
    g, ng = OL.group_table("large_pass2", 3, "cap960")
    assert ng == 65 and list(np.bincount(g)) == [960] + [1] * 64
    assert OL.loo_block_bytes(960) <= cap < OL.loo_block_bytes(961)
    g1, ng1 = OL.one_past("large_pass2", 3, "cap960")
    assert ng1 == 64 and list(np.bincount(g1)) == [961] + [1] * 63
    V = OL.directions("large_pass2", 0, 3)
    assert np.array_equal(V[:2], OL.directions("large_pass2", 0, 2)) and V.shape == (3, 36)


def test_every_entry_is_bound_to_inputs_rebuilt_from_seeds():
    """the SHA-256 of every entry matches (entry() raises otherwise), the truths have the shape of the call and are finite"""
    for e in OL.entries():
        r = OL.entry(e)
        H = T.num_hyp(*OL.fam(OL.base_case(e[1])))
        tj, tg = r["truth"]
        assert tg.shape == ((int(e[4][1:]), H) if e[3] == "fisher" else (H,)), e
        assert tg.dtype == X and np.all(np.isfinite(tg.astype(np.float64)))
        assert (tj is None) == (e[3] == "fisher") and (tj is None or np.isfinite(float(tj)))


def test_caps_and_conditioning():
    """the conditions on the inputs, on the errors of the CPU programs alone: M max(E_b, E_c) under both caps and cond(K) <= COND_MAX
    for every entry -- no min(budget, cap) rescue.  cond(K) is recomputed here for every (patient, draw)."""
    worst = {}
    conds = {}
    for e in OL.entries():
        r = OL.entry(e)
        _, _, bj, bg = OL.budgets(e)
        assert r["cond"] <= OL.COND_MAX, (e, r["cond"])
        assert bg <= OL.GRAD_BUDGET_CAP, (e, r["eg"], bg)
        if bj is not None:
            assert bj <= OL.NLML_BUDGET_CAP, (e, r["en"], bj)
        w = worst.setdefault(e[3], [0.0, 0.0, None])
        if bg > w[1]:
            worst[e[3]] = [max(w[0], bj or 0.0), bg, OL.key_of(e)]
        else:
            w[0] = max(w[0], bj or 0.0)
        ck = (e[1], e[2], OL.draw_of(*e[1:4]))
        if ck not in conds:
            conds[ck] = OL.cond_of(*e[1:4])
        assert abs(conds[ck] - r["cond"]) <= 1e-6 * r["cond"], (e, conds[ck], r["cond"])
    for obj, (bj, bg, key) in worst.items():
        print(f"OBJLARGE-CAPS {obj}: largest budget obj {bj:.3g} (cap {OL.NLML_BUDGET_CAP:.3g}), grad {bg:.3g} at {key} (cap {OL.GRAD_BUDGET_CAP:.3g})")


_BITS = [("pass2", "large_pass2", 0, "loo", "-"), ("pass2", "large_pass2", 0, "lgo", "cov"), ("pass2", "large_pass2", 0, "fc", "h6"),
         ("pass2", "large_pass2", 0, "fisher", "v2")]


@pytest.mark.parametrize("e", _BITS, ids=_ids(_BITS))
def test_stored_truth_bits(e):
    """one cheap entry per objective (n = 513): its long-double truth recomputed here equals hi + lo bit for bit"""
    assert e in OL.entries()
    r = OL.entry(e)
    tj, tg = OL.run_program(e, "truth")
    assert tg.dtype == X and np.array_equal(tg, r["truth"][1])
    assert tj is None or (tj == r["truth"][0] and r["truth"][0].dtype == X)


def test_one_group_is_the_nlml_truth():
    """table (b), one group of all 576 observations: the stored leave-group-out truth against nlml_truth's long-double nlml and
    gradient of the same inputs.  The two are different long-double programs (M_g = P is inverted again), so they agree to
    long-double rounding, not to the bit: the 64-bit significand has 11 bits on float64, and a float64 program of this entry errs by
    max(E_b, E_c); the two truths are demanded within 2^-8 of that (a factor of 8 for the longer operation chain)."""
    e = ("pass2", "large_pass2", 1, "lgo", "one")
    r = OL.entry(e)
    c = OL.case("large_pass2", "lgo")
    m, t, y = c["pts"][1]
    st, tn, tg = T.nlml_grad(*OL.fam(c), m, t, y, c["th"][1], X)
    dj = float(abs(r["truth"][0] - tn) / abs(tn))
    scale = np.maximum(np.abs(tg), X(1e-3) * np.abs(tg).max())
    dg = float((np.abs(r["truth"][1] - tg) / scale).max())
    print(f"OBJLARGE-ONEGROUP lgo truth against nlml truth: obj {dj:.3g} (E {max(r['en']):.3g}), grad {dg:.3g} (E {max(r['eg']):.3g})")
    assert st == 0 and dj <= max(max(r["en"]), OL.U64) / 256 and dg <= max(max(r["eg"]), OL.U64) / 256


_SMALL = [e for e in OL.entries() if OL.n_of(e[1], e[2]) <= 640]


@pytest.mark.parametrize("obj", OL.OBJECTIVES)
def test_float64_program_within_budget(obj):
    """the budget is satisfiable by a legitimate program: on every entry of n <= 640 the float64 run of the truth code, recomputed
    here against the STORED truth, stays within the budget.  It also has the stored error to a factor of 4: numpy's float64 products
    take another summation order with another BLAS thread count, which redraws the rounding noise the error is the maximum of
    (measured here with one thread against the stored errors: up to 1.7), while a stored truth that was off by more than an fp64
    rounding error would move the error by orders of magnitude -- the long double has 11 bits on float64"""
    rows = []
    for e in [e for e in _SMALL if e[3] == obj]:
        r = OL.entry(e)
        _, _, bj, bg = OL.budgets(e)
        ej, eg = OL.errors_of(e, OL.run_program(e, "b"), r["truth"])
        print(f"OBJLARGE-B {OL.key_of(e)}: obj {ej if ej is None else format(ej, '.3g')} (stored {r['en'] and r['en'][0]}), "
              f"grad {eg:.3g} (stored {r['eg'][0]:.3g}, budget {bg:.3g})")
        ok = eg <= bg and max(r["eg"][0], OL.U64) / 4 <= max(eg, OL.U64) <= 4 * max(r["eg"][0], OL.U64)
        if ej is not None:
            ok = ok and ej <= bj and max(r["en"][0], 4 * OL.U64) / 4 <= max(ej, 4 * OL.U64) <= 4 * max(r["en"][0], 4 * OL.U64)
        rows.append((OL.key_of(e), ok, ej, bj, eg, bg))
    assert rows and all(r[1] for r in rows), [r for r in rows if not r[1]]


@pytest.mark.parametrize("cid,p,h", [("lmc_sizes", 4, 6.0), ("lmc_sizes", 5, 0.0), ("lmc_sizes", 6, 6.0), ("sm_Q4", 0, 6.0)])
def test_shared_factor_forecast_truth_is_the_refit_truth(cid, p, h):
    """objective_large.forecast_grad_shared against forecast_grad_truth.forecast_grad (one factorisation per history length) in long
    double: the same bits, on patients of two to four 64-blocks"""
    c = FG.case(cid)
    m, t, y = c["pts"][p]
    pf = FG.prefix_of(c, p, h)
    a = FG.forecast_grad(*FG.fam(c), m, t, y, c["th"][p], pf, X)
    b = OL.forecast_grad_shared(*FG.fam(c), m, t, y, c["th"][p], pf, X)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and b[1].dtype == X


def test_fixture_fails_loudly():
    """an entry is bound to the bytes it was computed from: another table or a missing key raises, nothing is recomputed"""
    e = ("pass2", "large_pass2", 0, "lgo", "cov")
    g, ng = OL.group_table("large_pass2", 0, "cov")
    g2 = g.copy()
    g2[5] = (g2[5] + 1) % ng
    real = OL.group_table
    OL.group_table = lambda cid, p, s: (g2, ng)
    try:
        with pytest.raises(RuntimeError, match="other inputs"):
            OL.entry(e)
    finally:
        OL.group_table = real
    OL.entry(e)
    with pytest.raises(RuntimeError, match="holds no truth"):
        OL.entry(("pass2", "large_pass2", 0, "lgo", "one"))

