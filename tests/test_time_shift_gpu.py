"""The inference calls on the MI355X with the time axis moved to the documented limit |t| = 2^14 h (time_shift_cases.py): one
context per family, the patient re-uploaded at every offset of -2^14, 0, 2^10 and 2^14 h, one call per entry point, every output held
to the reference of the UNSHIFTED inputs -- the fp32 outputs by the existing checkers, the fp64 ones within
time_shift_cases.fp64_bounds (the quantity's existing bound, or the project's factor times what the fp64 table program loses at that
offset, recorded in tests/golden/time_shift_spread.json; never taken from device output) -- and the structural identities of the calls.
Every test prints the worst error per (call, family, offset) as TIMESHIFT-ERR lines (pytest -s).  tests/test_time_shift.py shows on the
CPU that a float32 phase at one test-side table site misses these bars by orders of magnitude."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
import components_ref as CR
import forecast_ref as FR
import functional_joint_ref as FJ
import functional_ref as FNR
import loo_ref as LR
import posterior_joint_ref as PJ
import posterior_ref as PR
import time_shift_cases as S
import trend_ref as TR


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(ctx, c, th, sh):
    """one call per entry point on the patients as uploaded: a dict per patient in the layout of time_shift_cases.restatements, the
    status words of every call, and the outputs only the identities need"""
    multi = c["kidx"] == 7
    P = len(sh)
    slots = np.arange(P)
    m2s = [q["m2"] for _, q in sh] if multi else None
    t2s = [q["t2"] for _, q in sh]
    packed = [q["packed"] if multi else (q["packed"][0], None, q["packed"][2], q["packed"][3]) for _, q in sh]
    status = {}
    post, status["posterior"] = ctx.posterior(slots, th, m2s, t2s)
    post0, status["posterior(parts=False)"] = ctx.posterior(slots, th, m2s, t2s, parts=False)
    joint, status["posterior_joint"], status["posterior_joint cov"] = ctx.posterior_joint(slots, th, m2s, t2s, [q["eps"] for _, q in sh])
    loo, status["loo"], gst = ctx.loo(slots, th, None)
    loo_cov, status["loo covariate"], gst_cov = ctx.loo(slots, th, "covariate")
    status["loo groups"] = np.concatenate(gst + gst_cov)
    fore, status["forecast"] = ctx.forecast(slots, th, m2s, t2s, [q["prefix"] for _, q in sh], [q["y2"] for _, q in sh])
    trend, status["trend"] = ctx.trend(slots, th, m2s, t2s)
    comp, status["components"] = ctx.components(slots, th, m2s, t2s)
    func, status["functionals"] = ctx.functionals(slots, th, packed)
    fjoint, status["functionals_joint"] = ctx.functionals_joint(slots, th, packed)
    lg = None
    if S.has_loo_grad(c):
        obj, grad, status["loo_grad"] = ctx.loo_grad(slots, th)
        lg = [(obj[p], grad[p]) for p in range(P)]
    # one point at every prefix 0 .. n of patient 0: var never rises with the prefix
    n = sh[0][0][1].shape[0]
    pf = np.arange(n + 1, dtype=np.int32)
    one, status["forecast prefixes"] = ctx.forecast([0], th[:1], [np.full(n + 1, sh[0][1]["m2"][0], np.int32)] if multi else None,
                                                   [np.full(n + 1, sh[0][1]["t2"][0], np.float32)], [pf])
    outs = []
    for p in range(P):
        outs.append({"posterior": post[p], "joint": joint[p], "samples": joint[p][3], "loo": loo[p], "loo_cov": loo_cov[p],
                     "loo_grad": lg[p] if lg else None, "forecast": fore[p], "trend": trend[p], "components": comp[p],
                     "functional": func[p], "functional_joint": fjoint[p]})
    return outs, status, dict(post0=post0, prefix_var=one[0][1])


def _hold(bad, what, fn):
    try:
        return fn()
    except AssertionError as e:
        bad.append((what, str(e)[:300]))


@pytest.mark.parametrize("name", S.FAMILIES)
def test_every_call_at_every_offset(name):
    c = S.case(name)
    kidx, Q, D, R = S.fam(c)
    P = len(c["pts"])
    th = np.stack(c["th"])
    ctx = medgp_amd.Context(kidx, Q, D, R)
    ctx.reserve(P, max(pt[1].shape[0] for pt in c["pts"]), P)
    bad = []
    for off in S.OFFSETS:
        sh = [S.shifted(name, p, off) for p in range(P)]
        for s, ((m, t, y), _) in enumerate(sh):
            ctx.set_patient(s, m if kidx == 7 else None, t, y)
        outs, status, extra = _run(ctx, c, th, sh)
        who = f"{name} offset {int(off)}"
        for call, st in status.items():
            if not np.all(st == 0):
                bad.append((who, call, "status", st.tolist()))
        worst32, worst64 = {}, {}
        for p in range(P):
            (m, t, y), q = sh[p]
            o, ref = outs[p], S.reference(name, p)
            m2 = q["m2"]
            w = f"{who} patient {p}"
            # ---- the fp32 outputs: the existing checkers, unchanged, against the unshifted reference
            _hold(bad, w + " posterior", lambda: PR.check_posterior(kidx, D, th[p], m2, ref["posterior"], *o["posterior"]))
            _hold(bad, w + " posterior_joint", lambda: PJ.check_joint(ref["joint"], o["joint"][1], o["joint"][2], o["joint"][3], q["eps"]))
            for key in ("loo", "loo_cov"):      # (lpd and total: the fp64 bound below; here the reference stands in for them)
                assert o[key][2].shape == ref[key][2].shape and o[key][2].dtype == np.float64
                _hold(bad, f"{w} {key}", lambda: LR.check_loo(ref[key], y, (o[key][0], o[key][1], ref[key][2], ref[key][3])))
            assert o["forecast"][2].shape == (S.M_POINTS,) and o["forecast"][2].dtype == np.float64
            _hold(bad, w + " forecast", lambda: FR.check_forecast(kidx, D, th[p], m2, q["prefix"], ref["forecast"][:2] + (None,),
                                                                  (o["forecast"][0], o["forecast"][1], None)))
            _hold(bad, w + " trend", lambda: TR.check_trend(kidx, D, th[p], m2, ref["trend"], o["trend"]))
            _hold(bad, w + " components", lambda: CR.check_components(Q, ref["components"], o["components"]))
            _hold(bad, w + " functionals", lambda: FNR.check_functional(ref["functional"], o["functional"]))
            _hold(bad, w + " functionals_joint", lambda: FJ.check_joint(ref["functional_joint"], o["functional_joint"]))
            # ---- the fp64 outputs
            e64 = S.fp64_errors(c, (m, t, y), o, ref)
            for k, b in S.fp64_bounds(name, p, off).items():
                worst64[k] = max(worst64.get(k, (0.0, 0.0)), (e64[k], b))
                if not e64[k] <= b:
                    bad.append((w, k, e64[k], "bound", b))
            for k, x in S.fp32_errors(c, (m, t, y), o, ref).items():
                worst32[k] = max(worst32.get(k, 0.0), x)
            # ---- the identities of the calls hold wherever the time axis sits
            tr, p0, fj = o["trend"], extra["post0"][p], o["functional_joint"]
            if not (np.array_equal(_bits(tr[0]), _bits(p0[0])) and np.array_equal(_bits(tr[1]), _bits(p0[1]))):
                bad.append((w, "the trend's mean / var do not have the bits of the posterior call's"))
            if not (np.array_equal(_bits(o["functional"][1]), _bits(np.diag(fj[2]))) and np.array_equal(_bits(o["functional"][0]), _bits(fj[0]))):
                bad.append((w, "fvar does not have the bits of diag(fcov)"))
        pv = extra["prefix_var"].astype(np.float64)
        if not (np.all(np.diff(pv) <= 0.0) and pv[0] > pv[-1]):
            bad.append((who, "var rises with the prefix"))
        calls = sorted({k.split(".")[0] for k in worst32})
        for call in calls:
            print(f"TIMESHIFT-ERR {who} {call}: " + " ".join(f"{k.split('.')[1]} {x:.3f}" for k, x in sorted(worst32.items()) if k.split(".")[0] == call)
                  + " (fp32 ulps)")
        print(f"TIMESHIFT-ERR {who} fp64: " + " ".join(f"{k} {e:.3g} (bound {b:.3g})" for k, (e, b) in sorted(worst64.items())))
    ctx.close()
    assert not bad, f"{len(bad)} misses:\n" + "\n".join(" | ".join(str(x) for x in b) for b in bad)
