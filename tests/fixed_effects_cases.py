"""Inputs of tests/test_fixed_effects_bits_gpu.py and tests/golden/make_fixed_effects_parent.py: the mean and basis calls on the branches
that tests/objective_calls_cases.py (D = 2 / 9, p = 3, MARGINAL posterior only) does not reach -- column counts 1, above 16, above 32
and above 48 (waves 1 to 3 of the post kernels, the full packed triangles), the posterior in FIXED mode, an improper entry (mean), a
failed pivot and a legal zero column (basis), an entry without test points.  Every case is a case of mean_truth / basis_truth, so
the smallest shape the suite has for its branch, run as ONE ragged batch on one context with the route pinned:

  mean   se (D = 1), lmc_D24 (patients 0, 1, 0: the third entry with lam = 0 on a covariate it never observes -- improper, status -1,
         NaN rows, as test_mean_gpu's test_improper_entry_... sets it), lmc_D33, lmc_D64
  basis  sm_p1, lmc_D3_p17, lmc_D24_p33, lmc_D3_p64, and "singular": test_basis_gpu's five slots on lmc_D3_p16 -- its three patients,
         patient 1 with column 15 a copy of column 0 and both flat (the failed pivot: status -1), patient 1 with column 15 zero under
         lam = 0.05 (legal)
Per case six calls: *_nlml_grad in both modes with flag_grad 0 and 1, *_posterior in both modes with the truth modules' 24 points per
entry, entry 1 given no points.
"""
import numpy as np

import medgp_amd
import basis_truth as BT
import mean_truth as MT

COLS = {"mean": {"se": 1, "lmc_D24": 24, "lmc_D33": 33, "lmc_D64": 64},
        "basis": {"sm_p1": 1, "lmc_D3_p17": 17, "lmc_D24_p33": 33, "lmc_D3_p64": 64, "singular": 16}}
CASES = [(f, c) for f in ("mean", "basis") for c in COLS[f]]
CALLS = [f"nlml_grad/{m}/{fg}" for m in ("marginal", "fixed") for fg in (0, 1)] + ["posterior/marginal", "posterior/fixed"]
EMPTY = 1     # the entry without test points


def setup(family, cid):
    """dict(fam, pts, H (None for mean), th, b0, lam, m2 (None off LMC-SM), t2, h2 (None for mean), ncol, status: the MARGINAL statuses
    the case claims)"""
    if family == "mean":
        c = MT.case(cid)
        ps = [0, 1, 0] if cid == "lmc_D24" else list(range(len(c["pts"])))
        lam = np.stack([c["lam"][p] for p in ps])
        status = [0] * len(ps)
        if cid == "lmc_D24":
            absent = int(np.where(np.bincount(c["pts"][0][0], minlength=c["D"]) == 0)[0][0])
            assert lam[2, absent] > 0
            lam[2, absent] = 0.0
            status[2] = -1
        pp = [MT.points(c, p) for p in ps]
        Hs, h2, T, ncol = None, None, MT, MT.nout(c["kidx"], c["D"])
    else:
        c = BT.case("lmc_D3_p16" if cid == "singular" else cid)
        ps = [0, 1, 2, 1, 1] if cid == "singular" else list(range(len(c["pts"])))
        Hs = [c["H"][p].copy() for p in ps]
        lam = np.stack([c["lam"][p] for p in ps])
        status = [0] * len(ps)
        if cid == "singular":
            Hs[3][:, 15] = Hs[3][:, 0]
            lam[3, [0, 15]] = 0.0
            status[3] = -1
            Hs[4][:, 15] = 0.0
            lam[4, 15] = 0.05
        pp = [BT.points(c, p) for p in ps]
        h2, T, ncol = [x[2] for x in pp], BT, c["p"]
    m2, t2 = ([x[0] for x in pp] if c["kidx"] == 7 else None), [x[1] for x in pp]
    z = np.zeros(0)
    t2[EMPTY] = z.astype(np.float32)
    if m2 is not None:
        m2[EMPTY] = z.astype(np.int32)
    if h2 is not None:
        h2[EMPTY] = np.zeros((0, ncol))
    return dict(fam=T.fam(c), pts=[c["pts"][p] for p in ps], H=Hs, th=np.stack([c["th"][p] for p in ps]),
                b0=np.stack([c["b0"][p] for p in ps]), lam=lam, m2=m2, t2=t2, h2=h2, ncol=ncol, status=status)


def flat(x):
    """every array of a (nested) result, in a fixed order"""
    if isinstance(x, np.ndarray):
        return [x]
    if isinstance(x, dict):
        return [a for k in sorted(x) for a in flat(x[k])]
    if isinstance(x, (list, tuple)):
        return [a for y in x for a in flat(y)]
    return []


def run(family, cid):
    """{call: (arrays of the result, its statuses)} of a case, on one fresh context with the route pinned"""
    s = setup(family, cid)
    ctx = medgp_amd.Context(*s["fam"])
    nb = len(s["pts"])
    ctx.reserve(nb, max(p[1].shape[0] for p in s["pts"]), nb)
    for k, (m, t, y) in enumerate(s["pts"]):
        ctx.set_patient(k, m if s["fam"][0] == 7 else None, t, y)
    if s["H"] is not None:
        ctx.set_basis(np.arange(nb), s["H"])
    ctx.pin_route(True)
    grad, post = getattr(ctx, family + "_nlml_grad"), getattr(ctx, family + "_posterior")
    pargs = (s["m2"], s["t2"]) + ((s["h2"],) if family == "basis" else ())
    out = {}
    try:
        for mode in ("marginal", "fixed"):
            kw = dict(b0=s["b0"], fixed=True) if mode == "fixed" else dict(b0=s["b0"], lam=s["lam"])
            for fg in (0, 1):
                r = grad(np.arange(nb), s["th"], flag_grad=bool(fg), **kw)
                out[f"nlml_grad/{mode}/{fg}"] = (flat(r), r["status"])
            r = post(np.arange(nb), s["th"], *pargs, **kw)
            out[f"posterior/{mode}"] = (flat(r), r[2])
    finally:
        ctx.close()
    return out
