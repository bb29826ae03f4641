"""The inputs of the time-shift GPU tests (time_shift_cases.py) without a GPU: the references do not move with the time axis, a
correct table program stays far inside the fp32 bar on exactly these inputs, what such a program loses in the fp64 outputs is the
committed record, and a float32 test-point phase is rejected."""
import json

import numpy as np
import pytest

import loo_ref as LR
import posterior_joint_ref as PJ
import time_shift_cases as S

MOVED = [off for off in S.OFFSETS if off != 0.0]
PATIENTS = [(name, p) for name in S.FAMILIES for p in S.patients(name)]
IDS = [f"{name}-{p}" for name, p in PATIENTS]


def _flat(out):
    """[(key, index, array)] of a restatements() / tables_restate() result"""
    rows = []
    for k in sorted(out):
        if out[k] is None:
            continue
        v = out[k] if isinstance(out[k], tuple) else (out[k],)
        rows += [(k, i, np.asarray(a)) for i, a in enumerate(v) if a is not None]
    return rows


def test_inputs_are_on_the_grid_and_cover_the_paths():
    for name, p in PATIENTS:
        c = S.case(name)
        m, t, y = c["pts"][p]
        q = S.call_inputs(name, p)
        for a in (t, q["t2"], q["packed"][2]):
            assert np.all(a * S.GRID == np.round(a * S.GRID)) and a.min() >= -3.0 and a.max() <= 203.0
        n = t.shape[0]
        assert q["t2"].shape == (S.M_POINTS,) and q["packed"][0].shape == (S.N_FUNCTIONALS + 1,) and q["eps"].shape == (S.M_POINTS, S.N_SAMPLES)
        assert q["prefix"].min() == 0 and q["prefix"].max() == n
        for off in S.OFFSETS:       # every shift is exact in float32 (asserted inside) and reaches the documented limit
            pt, qs = S.shifted(name, p, off)
            assert np.array_equal(pt[1].astype(np.float64) - off, t.astype(np.float64))
            assert np.array_equal(qs["t2"].astype(np.float64) - off, q["t2"].astype(np.float64))
    assert {S.case(n)["pts"][p][1].shape[0] for n, p in PATIENTS} >= {60, 120}      # one and two 64-row panels
    assert S.case("q17")["Q"] == 17 and S.case("sm")["kidx"] == 8 and S.case("se")["kidx"] == 0


@pytest.mark.parametrize("name,p", PATIENTS, ids=IDS)
def test_references_do_not_move_with_the_time_axis(name, p):
    """2a: every restatement forms tau from fp64 (or long double) differences of the float32 times, which are exact on the grid: the
    inputs moved by every offset give the bits of the unshifted run.  (The ones that go through the oracle's Gram matrix too: it takes
    (double) t_i - (double) t_j.)  The inputs are also as well conditioned as the checkers ask."""
    c = S.case(name)
    ref = S.reference(name, p)
    assert PJ.cond(ref["joint"][2]) <= PJ.COND_MAX
    assert LR.cond(LR.gram(*S.fam(c), c["pts"][p][0], c["pts"][p][1], c["th"][p])) <= PJ.COND_MAX
    for off in MOVED:
        pt, q = S.shifted(name, p, off)
        got = S.restatements(c, p, pt, q)
        a, b = _flat(ref), _flat(got)
        assert [(k, i) for k, i, _ in a] == [(k, i) for k, i, _ in b]
        for (k, i, x), (_, _, z) in zip(a, b):
            assert x.dtype == z.dtype and np.array_equal(x, z, equal_nan=True), (off, k, i)


@pytest.fixture(scope="module")
def table_runs():
    cache = {}

    def run(name, p, off):
        if (name, p, off) not in cache:
            cache[(name, p, off)] = S.tables_restate(name, p, off)
        return cache[(name, p, off)]
    return run


@pytest.mark.parametrize("name,p", PATIENTS, ids=IDS)
def test_table_program_leaves_room_under_the_fp32_bar(name, p, table_runs):
    """2b: every fp32 output of every call, formed from cos / sin tables at the shifted times in fp64, within 0.25 fp32 ulp of
    max(|ref|, 1e-3 S) of the reference at every offset: one eighth of the 2-ulp bar the device is held to"""
    c = S.case(name)
    ref = S.reference(name, p)
    worst = {}
    for off in S.OFFSETS:
        e = S.fp32_errors(c, c["pts"][p], table_runs(name, p, off), ref)
        k = max(e, key=e.get)
        worst[off] = (k, e[k])
        print(f"TIMESHIFT-ROOM {name}:{p} offset {int(off)}: worst {k} {e[k]:.4f} fp32 ulps")
    bad = {off: w for off, w in worst.items() if not w[1] <= S.ROOM}
    assert not bad, bad


def test_fp64_loss_is_the_committed_record(table_runs):
    """2c: the errors of the table program in the fp64 outputs, per (family, offset), re-derived and compared with
    tests/golden/time_shift_spread.json to within a factor of 2 (both floored at SPREAD_FLOOR)"""
    rec = json.load(open(S.GOLDEN))["spread"]
    assert sorted(rec) == sorted(S.FAMILIES)
    bad = []
    for name in S.FAMILIES:
        c = S.case(name)
        assert sorted(rec[name]) == sorted(S.off_key(off) for off in S.OFFSETS)
        for off in S.OFFSETS:
            now = {}
            for p in S.patients(name):
                for k, x in S.fp64_errors(c, c["pts"][p], table_runs(name, p, off), S.reference(name, p)).items():
                    now[k] = max(now.get(k, 0.0), x)
            r = rec[name][S.off_key(off)]
            assert sorted(r) == sorted(now), (name, off)
            for k in now:
                a, b = max(now[k], S.SPREAD_FLOOR[k]), max(r[k], S.SPREAD_FLOOR[k])
                if not (a <= 2 * b and b <= 2 * a):
                    bad.append((name, off, k, now[k], r[k]))
    assert not bad, bad


def test_fp64_bounds_come_from_the_record_and_never_fall_below_the_existing_ones():
    import forecast_ref as FR
    for name, p in PATIENTS:
        for off in S.OFFSETS:
            b = S.fp64_bounds(name, p, off)
            assert b["forecast_lpd"] >= FR.lpd_bound() and b["loo_lpd"] >= LR.LPD_BOUND
            assert ("loo_obj" in b) == S.has_loo_grad(S.case(name))
    # at the one-hour period the loss at 2^14 h is what sets the forecast bound: the reason the header states it as a function of |t|
    assert S.fp64_bounds("T1h", 0, 2.0 ** 14)["forecast_lpd"] > 10 * FR.lpd_bound()
    assert S.fp64_bounds("T72h", 0, 0.0)["forecast_lpd"] == FR.lpd_bound()


@pytest.mark.parametrize("off", [-2.0 ** 14, 2.0 ** 14])
@pytest.mark.parametrize("name", ["T1h", "T12h"])
def test_check_rejects_a_float32_test_point_phase(name, off):
    """2d: the table program with the test-point phase w t* rounded to float32 (what a float product or a sincosf at one of the
    test-side table sites gives) misses the 2-ulp bar at +-2^14 h, at the 1 h and the 12 h period, on every call whose test side reads
    tables: the GPU test has teeth on exactly these inputs"""
    import components_ref as CR
    import forecast_ref as FR
    import functional_joint_ref as FJ
    import functional_ref as FNR
    import posterior_ref as PR
    import trend_ref as TR
    c = S.case(name)
    p = 1
    ref = S.reference(name, p)
    pt, q = S.shifted(name, p, off)
    th, m2 = c["th"][p], q["m2"]
    f32 = (lambda a: np.asarray(a, np.float64).astype(np.float32))
    for phase32 in (False, True):
        out = S.tables_restate(name, p, off, phase32=phase32)
        checks = [
            lambda: PR.check_posterior(c["kidx"], c["D"], th, m2, ref["posterior"], *(f32(a) for a in out["posterior"])),
            lambda: PJ.check_joint(ref["joint"], f32(out["joint"][1]), f32(out["joint"][2])),
            lambda: FR.check_forecast(c["kidx"], c["D"], th, m2, q["prefix"], ref["forecast"][:2] + (None,), (f32(out["forecast"][0]), f32(out["forecast"][1]), None)),
            lambda: TR.check_trend(c["kidx"], c["D"], th, m2, ref["trend"], tuple(f32(a) for a in out["trend"][:5])),
            lambda: CR.check_components(c["Q"], ref["components"], _components_f32(out["components"])),
            lambda: FNR.check_functional(ref["functional"], tuple(f32(a) for a in out["functional"][:2])),
            lambda: FJ.check_joint(ref["functional_joint"], _fjoint_f32(out["functional_joint"])),
        ]
        for chk in checks:
            if phase32:
                with pytest.raises(AssertionError, match="beyond 2 fp32 ulps"):
                    chk()
            else:
                chk()       # the unmutated table program passes the same checkers


def _components_f32(o):
    """(cmean, cvar, ccov) as a device would write them: ccov rounded once, its diagonal the bits of cvar"""
    cc = np.asarray(o[2], np.float64).astype(np.float32)
    Q = cc.shape[1]
    return np.asarray(o[0]).astype(np.float32), np.ascontiguousarray(cc[:, np.arange(Q), np.arange(Q)]), cc


def _fjoint_f32(o):
    fc = np.asarray(o[2], np.float64).astype(np.float32)
    return np.asarray(o[0]).astype(np.float32), np.ascontiguousarray(np.diag(fc)), fc
