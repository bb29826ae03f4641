"""Inputs of tests/test_objective_calls_gpu.py and tests/golden/make_objective_calls_parent.py: three families at the smallest shapes
that reach every branch of the host helpers the derivative calls share (medgp_capi.hip: launch_slabsum / launch_epilogue,
factor_run_templated, launch_kinv, launch_kdot, ...), and the list of calls made on them.

  A = LMC-SM (7, 2, 2, 2), N = (40, 130, 70), the second patient uploaded interleaved: 1, 3 and 2 blocks of 64, which the plan
      (call_plan.h: size_bucket) puts into THREE size classes of one entry each; a non-identity permutation (forecast_grad's switched
      prefixes, lgo_grad's permuted group ids); a group of more than 64 members in the N = 130 patient.
      tests/test_inference_buffers_gpu.py's data plus one patient.
  B = LMC-SM (7, 9, 9, 2), N = (40, 70): Q in 9 .. 16 (two launches at every site that splits Q), H = 270 > 256 with few entries
      (two parts in the gradient epilogue); two classes of one entry.
  R = A's family, N = (40, 130, 200), the second patient interleaved: 1, 3 and 4 blocks, buckets 0, 2, 2 -- TWO size classes, one of them
      ragged (two entries of 4 and 3 blocks): its tile grids take the odd entry stride nbp = 2 | 1 = 3, and slab sums and epilogue run
      with more than one entry.  The group above 64 and the permutation are in the ragged class.
PLAN gives the size classes of each family, largest first, as (entries, 64-blocks of the largest); plan_of restates the rule on the CPU.
"""
import numpy as np

import medgp_amd
from medgp_amd import synth

FAMILIES = {"A": ((7, 2, 2, 2), (40, 130, 70)), "B": ((7, 9, 9, 2), (40, 70)), "R": ((7, 2, 2, 2), (40, 130, 200))}
PLAN = {"A": [(1, 3), (1, 2), (1, 1)], "B": [(1, 2), (1, 1)], "R": [(2, 4), (1, 1)]}


def plan_of(ns):
    """the size classes of a call on patients of ns observations (call_plan.h: blocks64, size_bucket; far below any cap on a class's
    entries or memory): [(entries, 64-blocks of the largest)], largest first"""
    nb = sorted(((max(n, 1) + 63) // 64 for n in ns), reverse=True)
    bucket = lambda b: next(j for j in range(32) if (1 << j) >= b)
    out = []
    for b in nb:
        if out and bucket(out[-1][1]) == bucket(b):
            out[-1] = (out[-1][0] + 1, out[-1][1])
        else:
            out.append((1, b))
    return out


NVEC = NCOT = 2
M2 = 5          # test points per patient
PB = 3          # basis columns


def data(name):
    """(family, [(meta, t, y) per patient], theta [P, H], [basis [n, PB] per patient])"""
    fam, ns = FAMILIES[name]
    D = fam[2]
    pts = [synth.patient(11, p, D, n, interleave=(name != "B" and p == 1)) for p, n in enumerate(ns)]
    th = np.stack([synth.theta(11, p, *fam) for p in range(len(ns))])
    Hs = [np.stack([np.ones(t.shape[0]), t.astype(np.float64) / 200.0, (m == 0).astype(np.float64)], axis=1) for m, t, _ in pts]
    return fam, pts, th, Hs


def make_ctx(name):
    """a fresh context with the family's patients and bases resident and every launch counted"""
    fam, pts, _, Hs = data(name)
    ctx = medgp_amd.Context(*fam)
    ctx.reserve(len(pts), max(p[1].shape[0] for p in pts), len(pts))
    for s, (m, t, y) in enumerate(pts):
        ctx.set_patient(s, m, t, y)
    ctx.set_basis(np.arange(len(pts)), Hs)
    ctx.profile_enable(True)
    return ctx


def _groups(ns):
    """as tests/test_inference_buffers_gpu.py: never held out, a singleton, an empty group (id 1), groups of 2 .. 64 and (N = 130) one
    of more than 64"""
    out = []
    for n in ns:
        gid = np.where(np.arange(n) % 3 == 0, 2, 3 + np.arange(n) % 4).astype(np.int32)
        gid[:3] = (-1, 0, -1)
        if n > 100:
            gid[30:100] = 7
        out.append(gid)
    return out


def calls(name):
    """[(call name, f(ctx) -> result)] in the order the test makes them on one context"""
    fam, pts, th, _ = data(name)
    ns = [p[1].shape[0] for p in pts]
    P, D, H = len(ns), fam[2], synth.num_hyp(*fam)
    slots = np.arange(P)
    g = np.random.default_rng(17)
    m2 = [g.integers(0, D, size=M2).astype(np.int32) for _ in ns]
    t2 = [g.uniform(0.0, 200.0, size=M2).astype(np.float32) for _ in ns]
    y2 = [g.normal(size=M2) for _ in ns]
    h2 = [np.stack([np.ones(M2), t.astype(np.float64) / 200.0, (m == 0).astype(np.float64)], axis=1) for m, t in zip(m2, t2)]
    vecs = g.normal(size=(P, NVEC, H))
    cm = [g.normal(size=(M2, NCOT)) for _ in ns]
    cv = [g.normal(size=(M2, NCOT)) for _ in ns]
    groups = _groups(ns)
    # observation i from the first prefix[i] <= i observations in upload order; every fifth one not scored
    prefix = [np.where(np.arange(n) % 5 == 4, -1, np.maximum(np.arange(n) - np.arange(n) % 4, 0)).astype(np.int32) for n in ns]
    mb0, mlam = 0.1 * g.normal(size=D), g.uniform(0.5, 2.0, size=D)
    bb0, blam = 0.1 * g.normal(size=PB), np.array([0.0, 1.0, 2.0])
    out = []
    for fg in (0, 1):
        out.append((f"loo_grad/{fg}", lambda c, fg=fg: c.loo_grad(slots, th, fg)))
    for fg in (0, 1):
        out.append((f"lgo_grad/{fg}", lambda c, fg=fg: c.lgo_grad(slots, th, groups, fg)))
    for fg in (0, 1):
        out.append((f"forecast_grad/{fg}", lambda c, fg=fg: c.forecast_grad(slots, th, prefix, fg)))
    out.append(("fisher_vec", lambda c: c.fisher_vec(slots, th, vecs)))
    out.append(("hess_vec", lambda c: c.hess_vec(slots, th, vecs)))
    out.append(("hess_vec/grad", lambda c: c.hess_vec(slots, th, vecs, want_grad=True)))
    out.append(("posterior_jvp", lambda c: c.posterior_jvp(slots, th, m2, t2, vecs)))
    out.append(("posterior_vjp/custom", lambda c: c.posterior_vjp(slots, th, m2, t2, cot_mean=cm, cot_var=cv)))
    out.append(("posterior_vjp/nlpd", lambda c: c.posterior_vjp(slots, th, m2, t2, loss="nlpd", y2_list=y2)))
    for what, b0, lam in (("mean", mb0, mlam), ("basis", bb0, blam)):
        for mode in ("marginal", "fixed"):
            kw = dict(b0=b0, fixed=True) if mode == "fixed" else dict(b0=b0, lam=lam)
            for fg in (0, 1):
                out.append((f"{what}_nlml_grad/{mode}/{fg}",
                            lambda c, what=what, kw=kw, fg=fg: getattr(c, what + "_nlml_grad")(slots, th, flag_grad=bool(fg), **kw)))
    out.append(("mean_posterior", lambda c: c.mean_posterior(slots, th, m2, t2, b0=mb0, lam=mlam)))
    out.append(("basis_posterior", lambda c: c.basis_posterior(slots, th, m2, t2, h2, b0=bb0, lam=blam)))
    out.append(("nlml_grad", lambda c: c.nlml_grad(slots, th, True)))
    return out


def flat(x):
    """every array of a (nested) result, in a fixed order"""
    if isinstance(x, np.ndarray):
        return [x]
    if isinstance(x, dict):
        return [a for k in sorted(x) for a in flat(x[k])]
    if isinstance(x, (list, tuple)):
        return [a for y in x for a in flat(y)]
    return [] if x is None else [np.atleast_1d(np.asarray(x))]


def statuses(name, res):
    """the per-patient status array of a call's result"""
    if isinstance(res, dict):
        return res["status"]
    if name.startswith("lgo_grad"):
        return res[2]
    if name in ("hess_vec/grad", "mean_posterior", "basis_posterior") or name.split("/")[0] in ("loo_grad", "forecast_grad", "nlml_grad"):
        return res[2]
    return res[1]      # fisher_vec, hess_vec, posterior_jvp, posterior_vjp


def run_one(ctx, f):
    """f on ctx with the launch counters reset before it: (arrays of the result, launch count per profile label, result, size classes
    of the call as (entries, 64-blocks of the largest))"""
    ctx.profile_reset()
    res = f(ctx)
    prof = ctx.profile_read()
    return flat(res), {k: int(v[1]) for k, v in prof.items()}, res, [c[:2] for c in ctx.last_plan()]


def run_fresh(name):
    """every call of the family on a context of its own: {call: (arrays, counts, result, plan)}"""
    out = {}
    for cname, f in calls(name):
        ctx = make_ctx(name)
        try:
            out[cname] = run_one(ctx, f)
        finally:
            ctx.close()
    return out
